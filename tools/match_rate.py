#!/usr/bin/env python3
"""Rate of the fixed-string match on IMIX traffic: nexg_match_batch over the
payloads and over the whole frames with sets of 1, 8 and 32 patterns, and
nexg_match_select on its rows, beside three passes over the same bytes in the
same process: Engine.probe_stream (the bare read), Engine.checksum (the
existing pass that also reads every byte) and the NEXG_OUT_RECORD parse.

The batch: --frames (default 4M) IMIX frames from Engine.gen_batch, packed,
with a u32 offset table. The generator's payloads are random bytes, so two
kinds of set fix the hit rate: "never" holds 8-byte ASCII patterns with
distinct first bytes (no frame carries one; one start position in 65536 per
pattern passes the two-byte prefilter), "half" the same with a one-byte
pattern in front, anywhere in the payload or from byte 64 on in the whole
frame (it occurs in few of the 64-byte frames and nearly all longer ones: near
40 % of the frames; a one-byte pattern passes the second
prefilter byte everywhere, so one position in 256 reaches the full compare).
Times are HIP events around `steps` back-to-back calls after 3 warm-up calls,
repeated --repeats times (all repeats are printed; the rates use the fastest).
Bytes per call, algorithmic: the match reads the region bytes once, the offset
table (4 B) and under the payload region two record dwords (8 B), and writes
8 B per frame. Rates are given as a fraction of 8 TB/s. One JSON line per
measurement.

usage: python tools/match_rate.py [--frames N] [--repeats R] [--quick]
"""
import argparse
import ctypes
import json
import os
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


def pattern_sets(whole):
    from nex_amd.match import Pattern
    never = [Pattern(b"%c-no-hit" % (0x41 + i)) for i in range(32)]  # 8 bytes, first bytes 'A'..'`'
    # over whole frames the one-byte pattern starts at byte 64 or later: the headers are full of zero bytes
    half = [Pattern(b"\x00", offset=(64, 65535) if whole else (0, 65535))] + never[:31]
    return {"never": never, "half": half}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 22)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--quick", action="store_true",
                    help="2 steps after 1 warm-up call, one repeat: the launches for a trace, not a timing")
    args = ap.parse_args()

    import torch
    from nex_amd import abi
    from nex_amd.engine import Engine
    from nex_amd.match import PatternSet
    if not torch.cuda.is_available():
        sys.exit("match_rate needs the GPU: no rate is reported without one")
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

    frame_bytes = b.total_bytes
    emit("probe_stream (read only)", lambda: eng.probe_stream(b.data, 0, stream=stream), 50,
         b.data.numel() // 16384 * 16384)
    emit("checksum_batch", lambda: eng.checksum(b, 0, stream=stream), 50, frame_bytes + n * 6)
    emit("record_parse", lambda: eng.parse(b, out_kind=abi.OUT_RECORD, out=recs, stream=stream), 50,
         frame_bytes + n * 64 + n * 4)
    h = recs.cpu().numpy().view(abi.RECORD_DTYPE)
    ok = ((h["flags"] >> abi.STATUS_SHIFT) & 7) == 0
    payload_bytes = int(h["payload_len"][ok].astype("int64").sum())
    del h

    rows = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
    idx = torch.empty(n, dtype=torch.int32, device="cuda")
    off = torch.empty(n, dtype=torch.int64, device="cuda")
    ln = torch.empty(n, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    wsb = abi.match_select_workspace(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")

    def select():
        rc = lib.nexg_match_select(ctx, ctypes.byref(fr), P(rows.data_ptr()), 1, 0, 0, P(idx.data_ptr()), P(off.data_ptr()),
                                   P(ln.data_ptr()), P(cnt.data_ptr()), P(ws.data_ptr()), wsb, st)
        assert rc == abi.OK

    for whole in (False, True):
        region = "frame" if whole else "payload"
        region_bytes = frame_bytes if whole else payload_bytes
        for kind, pats in pattern_sets(whole).items():
            for k in (1, 8, 32):
                pc = PatternSet(pats[:k], frame=whole).to_c()

                def match():
                    rc = lib.nexg_match_batch(ctx, ctypes.byref(fr), None if whole else P(recs.data_ptr()), ctypes.byref(pc),
                                              P(rows.data_ptr()), st)
                    assert rc == abi.OK

                match()
                select()
                hit = int(cnt.item())
                nbytes = region_bytes + n * (4 + 8 + (0 if whole else 8))
                emit("match_batch", match, 50, nbytes, region=region, set=kind, patterns=k, region_bytes=region_bytes,
                     first_pattern_hits=hit, hit_rate=round(hit / n, 4))
        # the selection on the last rows (the "half" set of 32): reads 8 B of row twice and the table, writes 16 B per kept frame
        emit("match_select (any = bit 0)", select, 50, 2 * n * 8 + n * 4 + hit * 16, region=region, selected=hit)


if __name__ == "__main__":
    main()
