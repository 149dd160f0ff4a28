#!/usr/bin/env python3
"""Rate of IPv4 reassembly on IMIX traffic: nexg_reasm_plan, nexg_reasm_frames
and nexg_reasm_held, beside nexg_fragment_plan / nexg_fragment_frames over the
same bytes in the same process.

The input is Engine.fragment of the generator's IMIX batch (--frames, default
1M) at mtu 576 under IGNORE_DF (every IPv4 frame of the mix over 576 bytes has
DF set: with DF honoured nothing would be split), its pieces put in a seeded random order (a
table gathered dense: the reassembly reads a packed batch, as a receive ring
gives it). The timing is that of tools/fragment_rate.py: HIP events around
`steps` back-to-back calls after warm-up calls, repeated --repeats times (all
repeats are printed; the rates use the fastest).

Bytes per call, algorithmic. Plan: the classification reads the table (8 B per
frame) and the header words (counted as 32 B) and writes 48 B per frame; each
of the eight radix passes reads its 8-B pairs twice and writes them once, with
histograms of 1 KiB per 1024 frames read and written twice (24 B + 4 B per
frame and pass); marks, places and rows read the order and the classifications
of two or three positions (counted as 4 + 2 x 32 + 8 + 32 + 2 x 32 B) and write
8 + 4 + 16 + 4 B per frame; the two scans read 20 B twice and write 12 + 4 B.
Fill: the frame bytes read once, the output bytes written once, 16 B of row and
20 B of prefixes read per frame and 16 B of table written per output frame.
Held: the row's kind read twice (16 B each, a whole row's sector) and 16 B
written per held frame. Rates are given as a fraction of 8 TB/s. One JSON line
per measurement.

usage: python tools/reasm_rate.py [--frames N] [--repeats R] [--quick]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MTU = 576
PLAN_BYTES_PER_FRAME = (8 + 32 + 48) + 8 * (24 + 4) + (4 + 64 + 8 + 32 + 64) + (8 + 4 + 16 + 4) + (2 * 20 + 16)


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
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--quick", action="store_true",
                    help="2 steps after 1 warm-up call, one repeat: the launches for a kernel trace, not a timing")
    args = ap.parse_args()

    import numpy as np
    import torch
    from nex_amd import abi
    from nex_amd.engine import Engine, FrameBatch
    from nex_amd.fragment import FragOption
    from nex_amd.reassemble import reassemble_host
    if not torch.cuda.is_available():
        sys.exit("reasm_rate needs the GPU: no rate is reported without one")
    eng = Engine(0)
    stream = torch.cuda.current_stream()
    P = ctypes.c_void_p
    st = P(stream.cuda_stream)
    lib, ctx = eng.lib, eng.ctx

    def emit(name, fn, steps, nbytes, **extra):
        ts = timed(fn, stream, 1, 2, 1) if args.quick else timed(fn, stream, 3, steps, args.repeats)
        best = min(ts)
        print(json.dumps(dict({"what": name, "steps": 2 if args.quick else steps, "ms": [round(x * 1e3, 4) for x in ts],
                               "bytes_per_call": int(nbytes), "tb_s": round(nbytes / best / 1e12, 4),
                               "frac_of_8tb_s": round(nbytes / best / 8e12, 4)}, **extra)), flush=True)
        return best

    # ---- the way out: the IMIX batch fragmented at mtu 576, timed as tools/fragment_rate.py times it
    packed = eng.gen_batch(abi.WL_IMIX, args.frames)
    n0, inner = packed.count, int(packed.data.numel())
    fc, oc = packed.to_c(), FragOption(MTU, abi.FRAG_IGNORE_DF).to_c()
    f_first = torch.empty(n0 + 1, dtype=torch.int32, device="cuda")
    f_bytes = torch.empty(n0 + 1, dtype=torch.int64, device="cuda")
    f_rows = torch.empty(n0 * 16, dtype=torch.uint8, device="cuda")
    fwsb = abi.fragment_plan_workspace(n0)
    fws = torch.empty(fwsb // 8 + 1, dtype=torch.int64, device="cuda")

    def fplan():
        assert lib.nexg_fragment_plan(ctx, ctypes.byref(fc), ctypes.byref(oc), P(f_first.data_ptr()), P(f_bytes.data_ptr()),
                                      P(f_rows.data_ptr()), P(fws.data_ptr()), fwsb, st) == abi.OK

    fplan()
    k, total = int(f_first[n0].item()) & 0xFFFFFFFF, int(f_bytes[n0].item())
    emit("fragment_plan", fplan, 1000, n0 * (2 * 8 + 2 * 16 + 12 + 16), frames=n0, mtu=MTU, output_frames=k)
    pieces = torch.empty(max(total, 16), dtype=torch.uint8, device="cuda")
    p_off = torch.empty(k + 1, dtype=torch.int64, device="cuda")
    p_len = torch.empty(max(k, 1), dtype=torch.int32, device="cuda")
    p_src = torch.empty(max(k, 1), dtype=torch.int32, device="cuda")

    def ffill():
        assert lib.nexg_fragment_frames(ctx, ctypes.byref(fc), ctypes.byref(oc), P(f_first.data_ptr()), P(f_bytes.data_ptr()), k,
                                        P(p_off.data_ptr()), P(p_len.data_ptr()), P(p_src.data_ptr()), P(pieces.data_ptr()), total,
                                        st) == abi.OK

    t_ffill = emit("fragment_frames", ffill, 200, inner + total + n0 * 20 + k * 16, frames=n0, mtu=MTU, output_frames=k,
                   bytes_read=inner, bytes_written=total)

    # ---- the pieces in a seeded random order, dense
    perm = torch.from_numpy(np.random.default_rng(1).permutation(k)).cuda()
    mixed = eng.gather(FrameBatch(data=pieces[:total], count=k, offsets=p_off[:k][perm], lengths=p_len[:k][perm]))
    del pieces
    n = mixed.count
    mc = mixed.to_c()
    r_first = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    r_bytes = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    r_rows = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
    wsb = abi.reasm_plan_workspace(n)
    ws = torch.empty(wsb // 8 + 2, dtype=torch.int64, device="cuda")

    def plan():
        assert lib.nexg_reasm_plan(ctx, ctypes.byref(mc), 1, P(r_first.data_ptr()), P(r_bytes.data_ptr()), P(r_rows.data_ptr()),
                                   P(ws.data_ptr()), wsb, st) == abi.OK

    plan()
    ko, ototal = int(r_first[n].item()) & 0xFFFFFFFF, int(r_bytes[n].item())
    t_plan = emit("reasm_plan", plan, 100, n * PLAN_BYTES_PER_FRAME, frames=n, output_frames=ko, workspace_bytes=wsb)
    out = torch.empty(max(ototal, 16), dtype=torch.uint8, device="cuda")
    t_off = torch.empty(ko + 1, dtype=torch.int64, device="cuda")
    t_len = torch.empty(max(ko, 1), dtype=torch.int32, device="cuda")
    t_src = torch.empty(max(ko, 1), dtype=torch.int32, device="cuda")
    m_bytes = int(mixed.data.numel())

    def fill():
        assert lib.nexg_reasm_frames(ctx, ctypes.byref(mc), 1, P(r_rows.data_ptr()), P(r_first.data_ptr()), P(r_bytes.data_ptr()),
                                     ko, P(t_off.data_ptr()), P(t_len.data_ptr()), P(t_src.data_ptr()), P(out.data_ptr()), ototal,
                                     st) == abi.OK

    t_fill = emit("reasm_frames", fill, 200, m_bytes + ototal + n * 36 + ko * 16, frames=n, output_frames=ko, bytes_read=m_bytes,
                  bytes_written=ototal)
    idx, off, ln = eng._table(n)
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    hwsb = abi.reasm_held_workspace(n)
    hws = torch.empty(hwsb // 8 + 1, dtype=torch.int64, device="cuda")

    def held():
        assert lib.nexg_reasm_held(ctx, ctypes.byref(mc), P(r_rows.data_ptr()), n, P(idx.data_ptr()), P(off.data_ptr()),
                                   P(ln.data_ptr()), P(cnt.data_ptr()), P(hws.data_ptr()), hwsb, st) == abi.OK

    held()
    nh = int(cnt.item())
    t_held = emit("reasm_held", held, 1000, n * 32 + nh * 16, frames=n, held=nh)
    print(json.dumps({"what": "reassembly, plan + fill + held", "ms": round((t_plan + t_fill + t_held) * 1e3, 4),
                      "input_bytes": m_bytes, "input_gb_s": round(m_bytes / (t_plan + t_fill + t_held) / 1e9, 2),
                      "plan share": round(t_plan / (t_plan + t_fill + t_held), 3),
                      "reasm_frames / fragment_frames": round(t_fill / t_ffill, 3)}), flush=True)

    # a spot check against the host contract: the datagrams of the first 300 output frames
    torch.cuda.synchronize()
    rows = r_rows.cpu().numpy().view(abi.REASM_DTYPE)
    # (two datagrams of the mix that share addresses and identification hold each other: `held` says how many)
    assert nh == int((rows["kind"] == abi.REASM_HELD).sum()) and ko == int(np.isin(rows["kind"], (1, 2)).sum())
    md, mo = mixed.data.cpu().numpy(), mixed.offsets.cpu().numpy()
    ho, hs = t_off.cpu().numpy(), t_src.cpu().numpy().view(np.uint32)
    od = out.cpu().numpy()
    for f in range(min(ko, 300)):
        h = int(hs[f])
        members = [h] if rows["kind"][h] == abi.REASM_PASS else [int(i) for i in np.flatnonzero(rows["head"] == h)]
        want = reassemble_host([md[mo[i]:mo[i + 1]].tobytes() for i in members])[0]
        assert len(want) == 1 and od[ho[f]:ho[f + 1]].tobytes() == want[0], f


if __name__ == "__main__":
    main()
