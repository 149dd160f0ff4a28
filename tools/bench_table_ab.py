#!/usr/bin/env python3
"""In-process A/B of the table passes across library builds, in the manner of
bench_parse_ab.py: one batch (the rate tools': --frames IMIX frames, packed,
u32 offset table) and one set of buffers, every entry point called through
each library with HIP events around `steps` back-to-back calls after warm-up
calls, the libraries interleaved and the order alternated round by round.
Timed: nexg_select_batch with select_rate.py's three filters (as they stand,
with one family-6 rule, and with out_rule), nexg_decap_select,
nexg_match_select, nexg_gather_plan, nexg_encap_plan, nexg_flow_batch,
nexg_flow_partition, nexg_flow_groups and nexg_flow_table_merge. The tunnel
rows and match rows the two selects read are made up here (every fourth inner
class, random masks): both libraries see the same bytes. --check compares
every output of every library with the first one's, bit for bit. One JSON
line per entry point: the rounds' ms per call and, for the first library,
its median and spread (max - min), for the others median - first median.

usage: python tools/bench_table_ab.py --libs A.so,B.so [--frames N] [--check]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", required=True)
    ap.add_argument("--frames", type=int, default=1 << 22)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    import torch
    from nex_amd import _lib, abi
    from nex_amd.encap import Tunnel, TunnelSet
    from nex_amd.engine import Engine
    from nex_amd.flow import FlowOption
    from nex_amd.select import Filter, Rule
    libs = args.libs.split(",")
    engines = []
    for path in libs:
        _lib._lib, _lib.LIB_PATH = None, os.path.abspath(path)
        engines.append(Engine(0))
    s = torch.cuda.current_stream()
    st = ctypes.c_void_p(s.cuda_stream)

    def P(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    def dev(n, dtype):
        return torch.empty(max(n, 1), dtype=dtype, device="cuda")

    # inputs, made once with the first library
    e0 = engines[0]
    b = e0.gen_batch(abi.WL_IMIX, args.frames).with_offsets32()
    n = b.count
    fr = b.to_c()
    recs = e0.parse(b, out_kind=abi.OUT_RECORD)
    fo = FlowOption(symmetric=True)
    foc = fo.to_c()
    flows = e0.flow(b, recs, fo)
    order = e0.flow_sort(flows)
    groups, _, n_groups, _ = e0.flow_groups(b, recs, flows, fo, order=order)
    i = torch.arange(n, device="cuda", dtype=torch.int32)
    tunnels = torch.zeros(n, 4, dtype=torch.int32, device="cuda")
    tunnels[:, 0] = abi.TUN_VXLAN | ((i % 4) << 16)  # accepted, inner classes 0..3 in turn
    inner_off = torch.arange(n, device="cuda", dtype=torch.int64) * 64
    inner_len = (i % 1400) + 14
    g = torch.Generator(device="cuda").manual_seed(abi.DEFAULT_SEED)
    match_rows = torch.randint(0, 1 << 31, (n, 2), dtype=torch.int64, device="cuda", generator=g).to(torch.int32)
    tc = TunnelSet([Tunnel.vxlan(7, "10.0.0.1", "10.0.0.2")]).to_c()
    torch.cuda.synchronize()

    # outputs, shared by the libraries
    idx, off, ln, rule = dev(n, torch.int32), dev(n, torch.int64), dev(n, torch.int32), dev(n, torch.uint8)
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    wsb = max(abi.select_workspace(n), abi.gather_plan_workspace(n), abi.flow_partition_workspace(n, 8),
              abi.flow_groups_workspace(n), abi.flow_table_workspace(0, n_groups))
    ws = dev((wsb + 7) // 8, torch.int64)
    offs = dev(n + 1, torch.int64)
    flow_out = dev(n * 8, torch.uint8)
    first = dev(9, torch.int64)
    grp_rows, group_of = dev(n_groups * 32, torch.uint8), dev(n, torch.int32)
    table_out, slot = dev(n_groups * 64, torch.uint8), dev(n_groups, torch.int32)

    def call(e, name, *a):
        rc = getattr(e.lib, name)(e.ctx, *a)
        assert rc == abi.OK, (name, rc, e.lib.nexg_ctx_last_error(e.ctx))

    table = (P(idx), P(off), P(ln))
    lines = []  # (name, fn(engine), the tensors it writes)
    none6 = Rule.host("2001:db8::dead", "src")  # select_rate.py: an address no IMIX frame carries
    for fname, rules in (("dst port 0-1047", [Rule.port(0, 1047, "dst")]), ("proto 17 or 1", [Rule.proto(17), Rule.proto(1)]),
                         ("match all", [Rule.any()])):
        for variant, six, want_rule in (("", False, False), (" + family-6 rule", True, False), (" + out_rule", False, True)):
            fc = Filter(rules + ([none6] if six else [])).to_c()
            lines.append((f"select_batch {fname}{variant}",
                          lambda e, fc=fc, r=want_rule: call(e, "nexg_select_batch", ctypes.byref(fr), P(recs), ctypes.byref(fc),
                                                              *table, P(rule) if r else None, P(cnt), P(ws), wsb, st),
                          [idx, off, ln, cnt] + ([rule] if want_rule else [])))
    lines.append(("decap_select inner 0|2", lambda e: call(e, "nexg_decap_select", P(tunnels), P(inner_off), P(inner_len), n, 0b101,
                                                           *table, P(cnt), P(ws), wsb, st), [idx, off, ln, cnt]))
    lines.append(("match_select any=3 none=4", lambda e: call(e, "nexg_match_select", ctypes.byref(fr), P(match_rows), 3, 0, 4,
                                                              *table, P(cnt), P(ws), wsb, st), [idx, off, ln, cnt]))
    lines.append(("gather_plan align 1", lambda e: call(e, "nexg_gather_plan", ctypes.byref(fr), 1, P(offs), None, P(ws), wsb, st),
                  [offs]))
    lines.append(("gather_plan align 16", lambda e: call(e, "nexg_gather_plan", ctypes.byref(fr), 16, P(offs), P(ln), P(ws), wsb, st),
                  [offs, ln]))
    lines.append(("encap_plan vxlan align 1", lambda e: call(e, "nexg_encap_plan", ctypes.byref(fr), ctypes.byref(tc), None, 1, P(offs),
                                                             P(ln), P(ws), wsb, st), [offs, ln]))
    lines.append(("flow_batch", lambda e: call(e, "nexg_flow_batch", ctypes.byref(fr), P(recs), ctypes.byref(foc), P(flow_out), st),
                  [flow_out]))
    lines.append(("flow_partition 8", lambda e: call(e, "nexg_flow_partition", ctypes.byref(fr), P(flows), 8, *table, P(first), P(ws),
                                                     wsb, st), [idx, off, ln, first]))
    lines.append(("flow_groups", lambda e: call(e, "nexg_flow_groups", ctypes.byref(fr), P(recs), P(flows), ctypes.byref(foc), P(order),
                                                P(grp_rows), n_groups, P(group_of), P(cnt), P(ws), wsb, st),
                  [grp_rows, group_of, cnt]))
    lines.append(("flow_table_merge into empty", lambda e: call(e, "nexg_flow_table_merge", ctypes.byref(fr), P(recs), ctypes.byref(foc),
                                                                P(groups), n_groups, None, 0, 1, 0, P(table_out), n_groups, P(slot),
                                                                P(cnt), P(ws), wsb, st), [table_out, slot, cnt]))

    for name, fn, outs in lines:
        if args.check:
            ref = None
            for lib, e in zip(libs, engines):
                for t in outs:
                    t.zero_()
                fn(e)
                torch.cuda.synchronize()
                got = [t.clone() for t in outs]  # rows past a selected count stay zero
                ref = got if ref is None else ref
                assert all(torch.equal(x, y) for x, y in zip(got, ref)), f"{name}: {lib} differs from {libs[0]}"
        times = {lib: [] for lib in libs}
        pairs = list(zip(libs, engines))
        for rnd in range(args.rounds):
            for lib, e in (pairs[::-1] if rnd % 2 else pairs):  # alternate the order (first-measured bias)
                for _ in range(args.warmup):
                    fn(e)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0.record(s)
                for _ in range(args.steps):
                    fn(e)
                t1.record(s)
                torch.cuda.synchronize()
                times[lib].append(round(t0.elapsed_time(t1) / args.steps, 4))
        base = times[libs[0]]
        med = statistics.median(base)
        print(json.dumps({"what": name, "frames": n, "checked": bool(args.check), "ms": times, "first_median": med,
                          "first_spread": round(max(base) - min(base), 4),
                          "median_minus_first": {lib: round(statistics.median(times[lib]) - med, 4) for lib in libs[1:]}}),
              flush=True)


if __name__ == "__main__":
    main()
