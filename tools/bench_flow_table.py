#!/usr/bin/env python3
"""Time of the flow-table merge (nexg_flow_table_merge) beside what bounds it
and what a caller pays anyway.

The batch: --frames (default 16M) generated IMIX frames, parsed to records, with
made-up flow rows: --flows (default 2^20) random 32-bit hashes dealt over the
frames at random, so the sort has work to do and the batch has about that
many groups. The table: --entries (default 2^20) entries ascending by hash,
half of their hashes taken from the batch's groups and half from elsewhere.

Three measurements, each in a child process of its own under its own time
limit (a measurement that fails or runs out of time ends the run; nothing is
started after it):

  merge  nexg_flow_table_merge of the batch's groups into the table
  copy   a device-to-device copy of (n_in + n_out) x 64 bytes, and one of half
         that size: the merge has to read table_in and write table_out once,
         which is the traffic of the smaller copy
  sort   nexg_flow_sort + nexg_flow_groups of the same batch, which a caller
         runs before every merge

Times are HIP events around back-to-back calls after warm-up calls (at least
--steps of them, and enough for a window of about 0.3 s), repeated --repeats
times (all repeats are printed; the rates use the fastest). At the default
sizes both tables together are 168 MB, less than the 256 MiB Infinity Cache, so
the copies and the merge's own table traffic run above the HBM rate.
One JSON line per measurement.

usage: python tools/bench_flow_table.py [--frames N] [--flows F] [--entries E]
                                        [--repeats R] [--steps S] [--window SECONDS] [--limit SECONDS]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, stream, warmup, steps, repeats, window=0.3):
    """Seconds per call, per repeat. `steps` is raised (to 5000 at most) until
    a repeat's timed window is about `window` seconds."""
    import torch
    out = []
    for r in range(repeats + 1):
        if r == 1:  # the first repeat only sizes the window
            steps = max(steps, min(5000, int(window / out.pop())))  # out.pop() > 0: a device time
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


def emit(what, times, nbytes, **more):
    best = min(times)
    print(json.dumps(dict({"what": what, "ms": [round(t * 1e3, 4) for t in times], "bytes": int(nbytes),
                           "tb_s": round(nbytes / best / 1e12, 4)}, **more)), flush=True)
    return best


def the_batch(args):
    """(engine, batch, records, flow rows) on the device."""
    import torch
    from nex_amd import abi
    from nex_amd.engine import Engine
    eng = Engine(0)
    batch = eng.gen_batch(abi.WL_IMIX, args.frames)
    recs = eng.parse(batch, out_kind=abi.OUT_RECORD)
    g = torch.Generator(device="cuda")
    g.manual_seed(args.seed)
    pool = torch.randint(0, 1 << 32, (args.flows,), dtype=torch.int64, device="cuda", generator=g)
    pick = torch.randint(0, args.flows, (args.frames,), dtype=torch.int64, device="cuda", generator=g)
    rows = pool[pick] | (abi.FLOW_IPV4_L4 << 32) | (17 << 40)  # hash, kind, proto
    return eng, batch, recs, rows.view(torch.uint8)


def run_sort(args):
    import torch
    from nex_amd import abi
    from nex_amd.engine import _ptr
    eng, batch, recs, flows = the_batch(args)
    n = batch.count
    lib, ctx, s = eng.lib, eng.ctx, eng._stream(None)
    fr = batch.to_c()
    order = torch.empty(n, dtype=torch.int32, device="cuda")
    out = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    gof = torch.empty(n, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    swb, gwb = abi.flow_sort_workspace(n), abi.flow_groups_workspace(n)
    sws, gws = eng._workspace(swb), eng._workspace(gwb)

    def call():
        rc = lib.nexg_flow_sort(ctx, _ptr(flows), n, _ptr(order), _ptr(sws), swb, s)
        rc = rc or lib.nexg_flow_groups(ctx, ctypes.byref(fr), _ptr(recs), _ptr(flows), None, _ptr(order), _ptr(out), n,
                                        _ptr(gof), _ptr(cnt), _ptr(gws), gwb, s)
        assert rc == abi.OK, lib.nexg_ctx_last_error(ctx)

    times = timed(call, torch.cuda.current_stream(), 1, args.steps, args.repeats, args.window)
    emit("flow_sort + flow_groups", times, 0, frames=n, groups=int(cnt.item()))


def run_merge(args):
    import torch
    from nex_amd import abi
    from nex_amd.engine import _ptr
    eng, batch, recs, flows = the_batch(args)
    groups, _, n_groups, _ = eng.flow_groups(batch, recs, flows)
    gh = groups.view(torch.int32).view(-1, 8)[:, 0].cpu().numpy().view(np.uint32)
    rng = np.random.default_rng(args.seed)
    shared = gh[::2][: args.entries // 2]
    fresh = np.setdiff1d(rng.integers(0, 1 << 32, 2 * args.entries, dtype=np.uint64).astype(np.uint32), gh)
    hashes = np.sort(np.concatenate([shared, fresh[: args.entries - len(shared)]]))
    table = np.zeros(len(hashes), abi.FLOW_ENTRY_DTYPE)
    table["hash"], table["last_epoch"], table["packets"], table["bytes"] = hashes, 1, 3, 300
    n_in, want = len(table), len(table) + n_groups - len(shared)
    t_in = torch.from_numpy(table.view(np.uint8).reshape(-1)).cuda()
    t_out = torch.empty(want * 64, dtype=torch.uint8, device="cuda")
    slot = torch.empty(n_groups, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    wsb = abi.flow_table_workspace(n_in, n_groups)
    ws = eng._workspace(wsb)
    lib, ctx, s = eng.lib, eng.ctx, eng._stream(None)
    fr = batch.to_c()

    def call():
        rc = lib.nexg_flow_table_merge(ctx, ctypes.byref(fr), _ptr(recs), None, _ptr(groups), n_groups, _ptr(t_in), n_in,
                                       2, 0, _ptr(t_out), want, _ptr(slot), _ptr(cnt), _ptr(ws), wsb, s)
        assert rc == abi.OK, lib.nexg_ctx_last_error(ctx)

    call()
    n_out = int(cnt.item())
    got = t_out.view(torch.int32).view(-1, 16)[:, 0].cpu().numpy().view(np.uint32)
    assert n_out == want and (np.diff(got.astype(np.int64)) > 0).all(), (n_out, want)
    times = timed(call, torch.cuda.current_stream(), 1, args.steps, args.repeats, args.window)
    emit("flow_table_merge", times, (n_in + n_out) * 64, frames=batch.count, n_groups=n_groups, n_in=n_in, n_out=n_out,
         shared=int(len(shared)), workspace_bytes=wsb)


def run_copy(args):
    import torch
    for what, nbytes in (("copy of (n_in + n_out) x 64 B", args.copy_bytes),
                         ("copy of half of it: the traffic of one read of table_in and one write of table_out",
                          args.copy_bytes // 2)):
        src = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        times = timed(lambda: dst.copy_(src), torch.cuda.current_stream(), 2, args.steps, args.repeats, args.window)
        emit(what, times, 2 * nbytes, copied=nbytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 24)
    ap.add_argument("--flows", type=int, default=1 << 20)
    ap.add_argument("--entries", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds a timed window should last (0: --steps calls)")
    ap.add_argument("--limit", type=int, default=240, help="seconds each measurement may take")
    ap.add_argument("--only", choices=("merge", "copy", "sort"),
                    help="one measurement in this process (what the children run; the way to put one under a profiler)")
    ap.add_argument("--copy-bytes", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.only:
        {"merge": run_merge, "copy": run_copy, "sort": run_sort}[args.only](args)
        return 0
    common = [sys.executable, os.path.abspath(__file__)] + [f"--{k}={getattr(args, k)}" for k in
                                                             ("frames", "flows", "entries", "repeats", "steps",
                                                              "seed", "window")]
    copy_bytes = 0
    for only in ("merge", "copy", "sort"):
        try:
            r = subprocess.run(common + ["--only", only, f"--copy-bytes={copy_bytes}"], capture_output=True, text=True,
                               timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(json.dumps({"what": only, "error": f"no result within {args.limit} s"}), flush=True)
            return 1
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            print(json.dumps({"what": only, "error": f"exit status {r.returncode}", "stderr": r.stderr[-2000:]}), flush=True)
            return 1
        if only == "merge":
            m = json.loads(r.stdout.splitlines()[-1])
            copy_bytes = (m["n_in"] + m["n_out"]) * 64
    return 0


if __name__ == "__main__":
    sys.exit(main())
