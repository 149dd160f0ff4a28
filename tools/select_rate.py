#!/usr/bin/env python3
"""Rate of the selection and gather passes on IMIX traffic: nexg_select_batch
(count + scan + scatter), nexg_gather_plan, nexg_gather_frames and
nexg_gather_rows on records, beside the NEXG_OUT_RECORD parse of the same
batch and a device-to-device copy of as many bytes as the gather moves (torch
copy_ in the same process: the ceiling the gather copy is judged against).

The batch: --frames (default 4M) IMIX frames from Engine.gen_batch, packed,
with a u32 offset table. Three filters set the selectivity: a destination-port
range (near 1 %), two protocol rules (UDP or ICMP, near 50 %) and match-all
(100 %); each select is timed as it stands (no frame byte is read) and with
one more rule on an IPv6 address no frame carries (every IPv6 frame's source
address is read from the frame). Times are HIP events around `steps`
back-to-back calls after warm-up calls, repeated --repeats times (all repeats
are printed; the rates use the fastest). Bytes per call, algorithmic: select
reads the flags word and the record dwords its rules test (4 B each) and the
offset table twice (count and scatter), plus 32 B per IPv6 frame under the
family-6 rule, and writes 16 B (17 with out_rule) per selected frame; the plan
reads the selected table (12 B) twice and writes 8 B per frame; the copy reads
and writes the selected bytes and reads the table and the planned offsets;
gather_rows reads 4 B of index and reads and writes 64 B per row. Rates are
given as a fraction of 8 TB/s. One JSON line per measurement.

usage: python tools/select_rate.py [--frames N] [--repeats R] [--quick]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, stream, warmup, steps, repeats):
    import torch
    out = []
    for _ in range(repeats):
        for _ in range(warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        for _ in range(steps):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / 1e3 / steps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 22)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--quick", action="store_true",
                    help="2 steps after 1 warm-up call, one repeat: the launches for a counter pass, not a timing")
    args = ap.parse_args()

    import torch
    from nex_amd import abi
    from nex_amd.engine import Engine, FrameBatch
    from nex_amd.select import Filter, Rule
    if not torch.cuda.is_available():
        sys.exit("select_rate needs the GPU: no rate is reported without one")
    eng = Engine(0)
    stream = torch.cuda.current_stream()
    b = eng.gen_batch(abi.WL_IMIX, args.frames).with_offsets32()
    n = b.count
    recs = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
    P = ctypes.c_void_p
    st = P(stream.cuda_stream)
    lib, ctx = eng.lib, eng.ctx
    fr = b.to_c()

    def emit(name, fn, steps, nbytes, **extra):
        ts = timed(fn, stream, 1, 2, 1) if args.quick else timed(fn, stream, 3, steps, args.repeats)
        best = min(ts)
        print(json.dumps(dict({"what": name, "frames": n, "steps": 2 if args.quick else steps,
                               "ms": [round(x * 1e3, 4) for x in ts], "bytes_per_call": int(nbytes),
                               "tb_s": round(nbytes / best / 1e12, 4), "frac_of_8tb_s": round(nbytes / best / 8e12, 4),
                               "mpkt_s": round(n / best / 1e6, 1)}, **extra)), flush=True)
        return best

    emit("record_parse", lambda: eng.parse(b, out_kind=abi.OUT_RECORD, out=recs, stream=stream), 20,
         b.total_bytes + n * 64 + n * 4)
    h = recs.cpu().numpy().view(abi.RECORD_DTYPE)
    v6_frames = int(((h["flags"] & abi.L_IPV6) != 0).sum())
    del h

    # one address no IMIX frame carries: the selectivity stays, the addresses are read
    none6 = Rule.host("2001:db8::dead", "src")
    filters = (("dst port 0-1047 (~1 %)", [Rule.port(0, 1047, "dst")], 2),
               ("proto 17 or 1 (~50 %)", [Rule.proto(17), Rule.proto(1)], 2),
               ("match all (100 %)", [Rule.any()], 1))
    idx = torch.empty(n, dtype=torch.int32, device="cuda")
    off = torch.empty(n, dtype=torch.int64, device="cuda")
    ln = torch.empty(n, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    wsb = abi.select_workspace(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    gws_b = abi.gather_plan_workspace(n)
    gws = torch.empty(gws_b // 8, dtype=torch.int64, device="cuda")
    goff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    rows = torch.empty(n * 64, dtype=torch.uint8, device="cuda")

    for name, rules, dwords in filters:
        for six in (False, True):
            fc = Filter(rules + ([none6] if six else [])).to_c()

            def select():
                rc = lib.nexg_select_batch(ctx, ctypes.byref(fr), P(recs.data_ptr()), ctypes.byref(fc), P(idx.data_ptr()),
                                           P(off.data_ptr()), P(ln.data_ptr()), None, P(cnt.data_ptr()), P(ws.data_ptr()),
                                           wsb, st)
                assert rc == abi.OK

            select()
            k = int(cnt.item())
            nbytes = 2 * n * (4 * dwords + 4) + k * 16 + (2 * (32 * v6_frames + 4 * n) if six else 0)
            emit("select_batch" + (" + one family-6 rule" if six else ""), select, 50, nbytes, filter=name, selected=k,
                 selectivity=round(k / n, 4))
        # gather of what the filter (with the family-6 rule: the same frames) selected
        sel = FrameBatch(data=b.data, count=k, offsets=off[:k], lengths=ln[:k], hints=abi.FRAMES_MONOTONE)
        sc = sel.to_c()

        def plan():
            rc = lib.nexg_gather_plan(ctx, ctypes.byref(sc), 1, P(goff.data_ptr()), None, P(gws.data_ptr()), gws_b, st)
            assert rc == abi.OK

        plan()
        total = int(goff[k].item())
        emit("gather_plan", plan, 50, k * (2 * 12 + 8), filter=name, selected=k)
        dense = torch.empty(max(total, 16), dtype=torch.uint8, device="cuda")

        def copy():
            rc = lib.nexg_gather_frames(ctx, ctypes.byref(sc), P(goff.data_ptr()), P(dense.data_ptr()), total, st)
            assert rc == abi.OK

        t_copy = emit("gather_frames", copy, 20, 2 * total + k * 20, filter=name, selected=k, bytes_copied=total)
        src = b.data[:total] if total else b.data[:16]
        dst = torch.empty_like(src)
        t_d2d = emit("device-to-device copy_ of as many bytes", lambda: dst.copy_(src), 20, 2 * src.numel(), filter=name)
        print(json.dumps({"what": "gather_frames / copy_ time ratio", "filter": name,
                          "ratio": round(t_copy / t_d2d, 3)}), flush=True)

        def gather_rows():
            rc = lib.nexg_gather_rows(ctx, P(recs.data_ptr()), 64, n, P(idx.data_ptr()), k, P(rows.data_ptr()), st)
            assert rc == abi.OK

        emit("gather_rows (records)", gather_rows, 50, k * (4 + 128), filter=name, selected=k)
        # the gathered batch is the selected frames, byte for byte (a spot check: first and last 1000)
        torch.cuda.synchronize()
        ho, hl, hg = off[:k].cpu().numpy(), ln[:k].cpu().numpy(), goff[: k + 1].cpu().numpy()
        for j in list(range(min(k, 1000))) + list(range(max(0, k - 1000), k)):
            a = b.data[int(ho[j]): int(ho[j]) + int(hl[j])]
            assert torch.equal(a, dense[int(hg[j]): int(hg[j]) + int(hl[j])]), j
        assert int(hg[k]) == int(np.sum(hl.astype(np.int64)))


if __name__ == "__main__":
    main()
