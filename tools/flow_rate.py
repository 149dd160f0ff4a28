#!/usr/bin/env python3
"""Rate of the flow passes on IMIX traffic: nexg_flow_batch (k_flow) and
nexg_flow_partition (count, the three-kernel scan, scatter) at 8 and 256
buckets, beside the NEXG_OUT_RECORD parse of the same batch and the
read + write stream ceiling nexg_probe_stream measures in the same process on
the same records (64 B read and 8 B written per frame: k_flow's own shape).

The batch: --frames (default 4M) IMIX frames from Engine.gen_batch, packed,
with a u32 offset table. Times are HIP events around `steps` back-to-back
calls after warm-up calls, repeated --repeats times (all repeats are printed;
the rates use the fastest). Bytes per call, algorithmic: k_flow reads the
64-B record and writes 8 B per frame, plus 4 B of offset table and 32 B of
addresses per IPv6 frame; the partition's count reads 8 B per frame (the flow
row; 4 B of it used) and writes buckets x tiles counters of 4 B; the scan
reads them twice and writes them once (plus the chunk sums); the scatter
reads the flow rows, 4 B of offset table and the counters again and writes
16 B per frame. One JSON line per measurement.

A flow_partition call is five kernels, so events give its whole time; the
three steps' own times come from a kernel trace of a --quick run:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python3 tools/flow_rate.py --quick
    python tools/flow_rate.py --steps-from DIR/.../run_kernel_trace.csv

which prints, per kernel and per bucket count (the dispatch order of a --quick
run), the median duration, the step it belongs to and the step's bytes.

--groups adds the per-flow counters on the same batch: nexg_flow_sort (with
the bytes of each of its four passes, and its time as a multiple of four
256-bucket partitions) and nexg_flow_groups at three flow populations: the
batch's own flows, and 1000 and 2^20 made-up hashes over the same records
(their members dealt round-robin over the batch, so the sort has work to do
and every group but the batch's own is a collision of many keys), each
against the stream ceiling per byte moved.

usage: python tools/flow_rate.py [--frames N] [--repeats R] [--quick] [--groups] [--steps-from CSV]
"""
import argparse
import csv
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BUCKETS = (8, 256)
STEP_OF = {"k_part_count": "count", "k_chunk_sums": "scan", "k_tile_scan": "scan", "k_chunk_apply": "scan",
           "k_part_scatter": "scatter"}
GROUP_KERNELS = ("k_sort_count", "k_sort_scatter", "k_group_mark", "k_group_place", "k_group_rows")


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


def step_bytes(n, buckets):
    """Algorithmic bytes of the partition's three steps for n frames."""
    from nex_amd import abi
    counters = (n + abi.FLOW_TILE - 1) // abi.FLOW_TILE * buckets
    chunks = (counters + 1023) // 1024
    return {"count": 8 * n + 4 * counters, "scan": 3 * 4 * counters + 3 * 4 * chunks,
            "scatter": 8 * n + 4 * n + 4 * counters + 16 * n}


def sort_pass_bytes(n):
    """Algorithmic bytes of the sort's four passes for n frames: a pass is the
    partition at 256 buckets on 8-B pairs (the first reads the flow rows, 8 B
    as well); its scatter writes 8 B per frame, the last one 4 B."""
    from nex_amd import abi
    counters = (n + abi.FLOW_TILE - 1) // abi.FLOW_TILE * 256
    chunks = (counters + 1023) // 1024
    return [{"count": 8 * n + 4 * counters, "scan": 3 * 4 * counters + 3 * 4 * chunks,
             "scatter": 8 * n + 4 * counters + (4 if p == 3 else 8) * n} for p in range(4)]


def groups_step_bytes(n, groups, v6_frames):
    """Algorithmic bytes of nexg_flow_groups for n frames in `groups` groups:
    mark reads 4 B of order, the 8-B flow row, the 64-B record and 4 B of
    offset table per position (plus 32 B of addresses per IPv6 frame), the
    record, table entry and addresses once more for every position that is not
    a group's first (the key of the position before), and writes 8 B; the
    three one-workgroup scans read and write 16 B per 256 positions; place
    reads 12 B and writes 4 B per position and 4 B per group; rows reads
    36 B and writes 32 B per group."""
    tiles = (n + 255) // 256
    per_key = 64 + 4 + 32 * v6_frames / max(n, 1)
    return {"mark": int(n * (4 + 8 + 8) + (2 * n - groups) * per_key), "scans": 2 * 16 * tiles,
            "place": 16 * n + 4 * groups, "rows": 68 * groups}


def steps_from(path, frames):
    """Median duration per partition kernel and bucket count from a kernel
    trace of a --quick run (dispatches alternate per bucket count in BUCKETS
    order: 1 warm-up + 2 timed calls each)."""
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            for k in list(STEP_OF) + ["k_flow"] + list(GROUP_KERNELS):
                if "nexg::" + k in name:
                    rows.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    if "k_flow" in rows:
        print(json.dumps({"what": "k_flow (trace)", "dispatches": len(rows["k_flow"]),
                          "median_us": round(float(np.median(rows["k_flow"])), 2)}))
    for bi, buckets in enumerate(BUCKETS):
        sb = step_bytes(frames, buckets)
        total = {}
        for k, step in STEP_OF.items():
            d = rows.get(k, [])[: 3 * len(BUCKETS)]  # a --groups run goes on to launch the scan kernels for the sort
            per = len(d) // len(BUCKETS)
            mine = d[bi * per: (bi + 1) * per]
            if not mine:
                continue
            med = float(np.median(mine))
            total[step] = total.get(step, 0.0) + med
            print(json.dumps({"what": k + " (trace)", "buckets": buckets, "step": step, "dispatches": len(mine),
                              "median_us": round(med, 2)}))
        for step, us in total.items():
            print(json.dumps({"what": "partition step (trace)", "buckets": buckets, "step": step, "us": round(us, 2),
                              "bytes": sb[step], "tb_s": round(sb[step] / us / 1e6, 4),
                              "frac_of_8tb_s": round(sb[step] / us / 8e6, 4)}))
    # a --quick --groups run: the sort's and the groups' own kernels; the groups' by flow population
    # (one checking call and three timed ones each, in the order of the run)
    for k in GROUP_KERNELS:
        d = rows.get(k, [])
        if not d:
            continue
        if k.startswith("k_sort"):
            print(json.dumps({"what": k + " (trace)", "dispatches": len(d), "median_us": round(float(np.median(d)), 2),
                              "sum_us_per_sort": round(float(np.median(d)) * 4, 2)}))
            continue
        per = len(d) // 3
        for pi in range(3):
            mine = d[pi * per: (pi + 1) * per]
            print(json.dumps({"what": k + " (trace)", "population": pi, "dispatches": len(mine),
                              "median_us": round(float(np.median(mine)), 2)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 22)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--quick", action="store_true",
                    help="2 steps after 1 warm-up call, one repeat: the launches for a trace or counter pass, not a timing")
    ap.add_argument("--groups", action="store_true",
                    help="also time nexg_flow_sort and nexg_flow_groups (per-flow counters) on the same batch")
    ap.add_argument("--steps-from", metavar="CSV", help="summarise the partition kernels of a rocprofv3 kernel trace")
    args = ap.parse_args()
    if args.steps_from:
        return steps_from(args.steps_from, args.frames)

    import torch
    from nex_amd import abi
    from nex_amd.engine import Engine
    from nex_amd.flow import FlowOption, flows_host, partition_host, sort_host
    if not torch.cuda.is_available():
        sys.exit("flow_rate needs the GPU: no rate is reported without one")
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
    ok = ((h["flags"] >> abi.STATUS_SHIFT) & 7) == 0
    v6_frames = int((ok & ((h["flags"] & abi.L_IPV6) != 0) & ((h["flags"] & abi.L_IPV4) == 0)).sum())

    # the ceiling for k_flow's shape: the records read, 8 B per 64 B written
    probe_out = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
    t_probe = emit("probe_stream (64 B read + 8 B written per frame: the ceiling)",
                   lambda: eng.probe_stream(recs, 8, out=probe_out, stream=stream), 50, n * 72)

    flows = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
    flow_bytes = n * (64 + 8 + 4) + 32 * v6_frames
    for name, opt in (("default", FlowOption()), ("symmetric", FlowOption(symmetric=True)),
                      ("no ports", FlowOption(ports=False))):
        fo = opt.to_c()

        def flow():
            rc = lib.nexg_flow_batch(ctx, ctypes.byref(fr), P(recs.data_ptr()), ctypes.byref(fo), P(flows.data_ptr()), st)
            assert rc == abi.OK

        t = emit("flow_batch (k_flow)", flow, 50, flow_bytes, option=name, ipv6_frames=v6_frames)
        print(json.dumps({"what": "k_flow time / probe_stream time, per byte moved", "option": name,
                          "ratio": round((t / flow_bytes) / (t_probe / (n * 72)), 3)}), flush=True)
    # leave the default rows in place for the partition, and spot-check them (first and last 1000)
    fo = FlowOption().to_c()
    assert lib.nexg_flow_batch(ctx, ctypes.byref(fr), P(recs.data_ptr()), ctypes.byref(fo), P(flows.data_ptr()), st) == abi.OK
    torch.cuda.synchronize()
    hf = flows.cpu().numpy().view(abi.FLOW_DTYPE)
    offs, data = b.host_offsets(), None
    for lo, hi in ((0, min(n, 1000)), (max(0, n - 1000), n)):
        data = b.data[int(offs[lo]): int(offs[hi])].cpu().numpy().tobytes()
        frames = [data[int(offs[i] - offs[lo]): int(offs[i + 1] - offs[lo])] for i in range(lo, hi)]
        want = flows_host(frames, h[lo:hi], [len(f) for f in frames])
        assert want.tobytes() == hf[lo:hi].tobytes(), "k_flow differs from flow_host"
    kinds = np.bincount(hf["kind"], minlength=5).tolist()
    print(json.dumps({"what": "flow kinds (none, v4, v4+l4, v6, v6+l4)", "frames": kinds}), flush=True)

    idx = torch.empty(n, dtype=torch.int32, device="cuda")
    off = torch.empty(n, dtype=torch.int64, device="cuda")
    ln = torch.empty(n, dtype=torch.int32, device="cuda")
    for buckets in BUCKETS:
        first = torch.empty(buckets + 1, dtype=torch.int64, device="cuda")
        wsb = abi.flow_partition_workspace(n, buckets)
        ws = torch.empty((wsb + 7) // 8, dtype=torch.int64, device="cuda")

        def part():
            rc = lib.nexg_flow_partition(ctx, ctypes.byref(fr), P(flows.data_ptr()), buckets, P(idx.data_ptr()),
                                         P(off.data_ptr()), P(ln.data_ptr()), P(first.data_ptr()), P(ws.data_ptr()), wsb,
                                         st)
            assert rc == abi.OK

        sb = step_bytes(n, buckets)
        t = emit("flow_partition (count + scan + scatter)", part, 50, sum(sb.values()), buckets=buckets, workspace_bytes=wsb,
             step_bytes=sb)
        torch.cuda.synchronize()
        want_idx, want_first = partition_host(hf["hash"], buckets)
        assert (idx.cpu().numpy().view(np.uint32) == want_idx).all(), "partition differs from partition_host"
        assert first.cpu().numpy().tolist() == want_first.tolist()
        sizes = np.diff(want_first)
        print(json.dumps({"what": "bucket sizes", "buckets": buckets, "min": int(sizes.min()), "max": int(sizes.max()),
                          "mean": round(float(sizes.mean()), 1)}), flush=True)
        if buckets == 256:
            t_part256 = t

    if not args.groups:
        return
    # ---- per-flow counters: nexg_flow_sort, then nexg_flow_groups at three flow populations
    order = torch.empty(n, dtype=torch.int32, device="cuda")
    swb = abi.flow_sort_workspace(n)
    sws = torch.empty(swb // 8, dtype=torch.int64, device="cuda")

    def sort(rows=flows):
        rc = lib.nexg_flow_sort(ctx, P(rows.data_ptr()), n, P(order.data_ptr()), P(sws.data_ptr()), swb, st)
        assert rc == abi.OK

    pb = sort_pass_bytes(n)
    t_sort = emit("flow_sort (4 x (count + scan + scatter))", sort, 20, sum(sum(p.values()) for p in pb),
                  workspace_bytes=swb, pass_bytes=pb)
    torch.cuda.synchronize()
    assert (order.cpu().numpy().view(np.uint32) == sort_host(hf["hash"])).all(), "flow_sort differs from sort_host"
    print(json.dumps({"what": "flow_sort time / four flow_partition calls at 256 buckets",
                      "ratio": round(t_sort / (4 * t_part256), 3)}), flush=True)

    gwb = abi.flow_groups_workspace(n)
    gws = torch.empty(gwb // 8, dtype=torch.int64, device="cuda")
    rows_out = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    group_of = torch.empty(n, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    i64 = np.arange(n, dtype=np.uint64)
    populations = [("the batch's own flows", flows)]
    for pop in (1000, 1 << 20):
        # the same records under made-up hashes: `pop` groups, their members dealt round-robin over the batch
        rows = hf.copy()
        rows["hash"] = ((i64 % np.uint64(pop)) * np.uint64(2654435761) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        populations.append((f"{pop} made-up hashes over the same records", torch.from_numpy(rows.view(np.uint8)).cuda()))
    for name, rows in populations:
        sort(rows)

        def groups():
            rc = lib.nexg_flow_groups(ctx, ctypes.byref(fr), P(recs.data_ptr()), P(rows.data_ptr()), ctypes.byref(fo),
                                      P(order.data_ptr()), P(rows_out.data_ptr()), n, P(group_of.data_ptr()),
                                      P(cnt.data_ptr()), P(gws.data_ptr()), gwb, st)
            assert rc == abi.OK

        groups()
        G = int(cnt.item())
        hr = rows.cpu().numpy().view(abi.FLOW_DTYPE)
        uniq, packets = np.unique(hr["hash"], return_counts=True)
        got = rows_out.cpu().numpy().view(abi.FLOW_GROUP_DTYPE)[:G]
        assert G == len(uniq) and (got["hash"] == uniq).all() and (got["packets"] == packets).all(), "flow_groups"
        lens = np.diff(offs[: n + 1])
        assert int(got["bytes"].sum()) == int(lens.sum()) and int(got["packets"].sum()) == n
        gb = groups_step_bytes(n, G, v6_frames)
        t = emit("flow_groups (mark + scans + place + rows)", groups, 20, sum(gb.values()), population=name, groups=G,
                 mixed_groups=int((got["mixed"] != 0).sum()), workspace_bytes=gwb, step_bytes=gb)
        print(json.dumps({"what": "flow_groups time / probe_stream time, per byte moved", "population": name,
                          "ratio": round((t / sum(gb.values())) / (t_probe / (n * 72)), 3)}), flush=True)


if __name__ == "__main__":
    main()
