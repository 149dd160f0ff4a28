#!/usr/bin/env python3
"""Rate of the header rewrite: nexg_rewrite_batch with a NAT44 + ports + DEC_TTL
action in RECOMPUTE and INCREMENTAL mode, beside the only route the library had
to the same checksum bytes on the device before it: nexg_recompute_checksums_batch
with which = IP | L4 on the same batch (which does not even make the edits).

Two batches of --frames (default 4M) frames from Engine.gen_batch: UDP64 at a
fixed 64-B stride and IMIX packed (u64 offsets). Times are HIP events around
`steps` back-to-back calls after 3 warm-up calls, repeated --repeats times (all
repeats are printed; the rates use the fastest). GB/s is frame bytes per call
over that time: the RECOMPUTE instance and the fix-up read every frame byte,
the INCREMENTAL instance reads header bytes only, so its GB/s on frame bytes
is a rate of frames, not of memory. Every step runs under its own time limit
(--limit seconds, SIGALRM): a step that outlives it ends the process with
status 124. One JSON line per measurement.

--pmc-run: no timing; 1 warm-up call and 3 calls of each rewrite instance and
of the fix-up on each batch, for a counter run of its own
(rocprofv3 --pmc FETCH_SIZE -- python3 tools/rewrite_rate.py --pmc-run). On
gfx950 FETCH_SIZE counts 64 B per 128-B request: double it.

usage: python tools/rewrite_rate.py [--frames N] [--repeats R] [--limit S] [--pmc-run]
"""
import argparse
import json
import os
import signal
import sys

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


def _expired(signum, frame):
    sys.stderr.write("rewrite_rate: a step outlived its time limit\n")
    os._exit(124)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 22)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=60, help="seconds a single step may take")
    ap.add_argument("--pmc-run", action="store_true")
    args = ap.parse_args()

    import torch
    from nex_amd import abi
    from nex_amd.engine import Engine
    from nex_amd.rewrite import Action, ActionSet
    if not torch.cuda.is_available():
        sys.exit("rewrite_rate needs the GPU: no rate is reported without one")
    signal.signal(signal.SIGALRM, _expired)
    eng = Engine(0)
    stream = torch.cuda.current_stream()
    nat = Action.nat4(src="192.0.2.1", dst="198.51.100.7") & Action.ports(40000, 443) & Action.dec_ttl(1)

    for name, wl in (("udp64 fixed stride", abi.WL_UDP64), ("imix packed", abi.WL_IMIX)):
        signal.alarm(args.limit)
        b = eng.gen_batch(wl, args.frames)
        torch.cuda.synchronize()
        frame_bytes = b.total_bytes
        steps = {
            "recompute_checksums (IP | L4), no edit": lambda: eng.recompute_checksums(b, report=False, stream=stream),
            "rewrite RECOMPUTE": lambda: eng.rewrite(b, ActionSet([nat]), report=False, stream=stream),
            "rewrite INCREMENTAL": lambda: eng.rewrite(b, ActionSet([nat], incremental=True), report=False, stream=stream),
        }
        for what, fn in steps.items():
            signal.alarm(args.limit)
            if args.pmc_run:
                for _ in range(4):
                    fn()
                torch.cuda.synchronize()
                print(json.dumps({"batch": name, "what": what, "frames": b.count, "frame_bytes": frame_bytes, "calls": 4}),
                      flush=True)
                continue
            ts = timed(fn, stream, 3, 20, args.repeats)
            best = min(ts)
            print(json.dumps({"batch": name, "what": what, "frames": b.count, "frame_bytes": frame_bytes,
                              "ms": [round(x * 1e3, 4) for x in ts], "gb_s_on_frame_bytes": round(frame_bytes / best / 1e9, 1),
                              "mpkt_s": round(b.count / best / 1e6, 1)}), flush=True)
        signal.alarm(0)
        del b
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
