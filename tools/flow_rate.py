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

usage: python tools/flow_rate.py [--frames N] [--repeats R] [--quick] [--steps-from CSV]
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


def steps_from(path, frames):
    """Median duration per partition kernel and bucket count from a kernel
    trace of a --quick run (dispatches alternate per bucket count in BUCKETS
    order: 1 warm-up + 2 timed calls each)."""
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            for k in list(STEP_OF) + ["k_flow"]:
                if "nexg::" + k in name:
                    rows.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    if "k_flow" in rows:
        print(json.dumps({"what": "k_flow (trace)", "dispatches": len(rows["k_flow"]),
                          "median_us": round(float(np.median(rows["k_flow"])), 2)}))
    for bi, buckets in enumerate(BUCKETS):
        sb = step_bytes(frames, buckets)
        total = {}
        for k, step in STEP_OF.items():
            d = rows.get(k, [])
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 22)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--quick", action="store_true",
                    help="2 steps after 1 warm-up call, one repeat: the launches for a trace or counter pass, not a timing")
    ap.add_argument("--steps-from", metavar="CSV", help="summarise the partition kernels of a rocprofv3 kernel trace")
    args = ap.parse_args()
    if args.steps_from:
        return steps_from(args.steps_from, args.frames)

    import torch
    from nex_amd import abi
    from nex_amd.engine import Engine
    from nex_amd.flow import FlowOption, flows_host, partition_host
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
        emit("flow_partition (count + scan + scatter)", part, 50, sum(sb.values()), buckets=buckets, workspace_bytes=wsb,
             step_bytes=sb)
        torch.cuda.synchronize()
        want_idx, want_first = partition_host(hf["hash"], buckets)
        assert (idx.cpu().numpy().view(np.uint32) == want_idx).all(), "partition differs from partition_host"
        assert first.cpu().numpy().tolist() == want_first.tolist()
        sizes = np.diff(want_first)
        print(json.dumps({"what": "bucket sizes", "buckets": buckets, "min": int(sizes.min()), "max": int(sizes.max()),
                          "mean": round(float(sizes.mean()), 1)}), flush=True)


if __name__ == "__main__":
    main()
