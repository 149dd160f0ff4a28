#!/usr/bin/env python3
"""Rate of IPv4 fragmentation on IMIX traffic: nexg_fragment_plan and
nexg_fragment_frames

  * at an mtu above every frame (9000: all pass-through, a one-to-one copy),
    beside Engine.gather's fill (nexg_gather_frames) and nexg_encap_frames
    (VXLAN over IPv4, no UDP checksum) over the same table in the same process;
  * on that VXLAN-encapsulated batch at mtu 1500, where the 1500-byte class
    (1550 bytes behind the outer header) splits in two.

The batch and the timing are those of tools/encap_rate.py: --frames (default
4M) IMIX frames from Engine.gen_batch, packed, with a u32 offset table; HIP
events around `steps` back-to-back calls after warm-up calls, repeated
--repeats times (all repeats are printed; the rates use the fastest). The
steps (200 fills, 1000 plans) make a timed window a third of a second or more.
Bytes per call, algorithmic: the plan reads the table (8 B per frame: two u32 offsets)
twice and the four header words of each frame (counted as 16 B) twice, and
writes 12 B of prefixes and the 16-B row per frame; the fill reads the frame
bytes once (a split frame's header once more per extra piece is not counted:
it comes from LDS) and writes the output bytes, and reads the table and the
two planned prefixes (8 + 4 + 8 B per frame, counted once: neighbours share a
cache line) and writes 16 B of table per output frame. Rates are given as a
fraction of 8 TB/s. One JSON line per measurement.

usage: python tools/fragment_rate.py [--frames N] [--repeats R] [--quick]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 22)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--quick", action="store_true",
                    help="2 steps after 1 warm-up call, one repeat: the launches for a counter pass, not a timing")
    args = ap.parse_args()

    import numpy as np
    import torch
    from nex_amd import abi
    from nex_amd.encap import Tunnel, TunnelSet
    from nex_amd.engine import Engine
    from nex_amd.fragment import FragOption, fragment_frame
    if not torch.cuda.is_available():
        sys.exit("fragment_rate needs the GPU: no rate is reported without one")
    eng = Engine(0)
    stream = torch.cuda.current_stream()
    packed = eng.gen_batch(abi.WL_IMIX, args.frames)
    b = packed.with_offsets32()
    n = b.count
    P = ctypes.c_void_p
    st = P(stream.cuda_stream)
    lib, ctx = eng.lib, eng.ctx

    def emit(name, fn, steps, nbytes, **extra):
        ts = timed(fn, stream, 1, 2, 1) if args.quick else timed(fn, stream, 3, steps, args.repeats)
        best = min(ts)
        print(json.dumps(dict({"what": name, "frames": n, "steps": 2 if args.quick else steps,
                               "ms": [round(x * 1e3, 4) for x in ts], "bytes_per_call": int(nbytes),
                               "tb_s": round(nbytes / best / 1e12, 4), "frac_of_8tb_s": round(nbytes / best / 8e12, 4)},
                              **extra)), flush=True)
        return best

    first = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    nbytes = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    rows = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
    wsb = abi.fragment_plan_workspace(n)
    ws = torch.empty(wsb // 8 + 1, dtype=torch.int64, device="cuda")

    def measure(label, batch, ho, mtu):
        """The plan and the fill of `batch` (its u64 offsets on the host: ho) at `mtu`; returns the fill's time, the
        input bytes and the output bytes."""
        fc, oc = batch.to_c(), FragOption(mtu).to_c()
        inner = int(batch.data.numel())

        def plan():
            rc = lib.nexg_fragment_plan(ctx, ctypes.byref(fc), ctypes.byref(oc), P(first.data_ptr()), P(nbytes.data_ptr()),
                                        P(rows.data_ptr()), P(ws.data_ptr()), wsb, st)
            assert rc == abi.OK

        plan()
        k, total = int(first[n].item()) & 0xFFFFFFFF, int(nbytes[n].item())
        emit("fragment_plan", plan, 1000, n * (2 * 8 + 2 * 16 + 12 + 16), case=label, mtu=mtu, output_frames=k)
        out = torch.empty(max(total, 16), dtype=torch.uint8, device="cuda")
        t_off = torch.empty(k + 1, dtype=torch.int64, device="cuda")
        t_len = torch.empty(max(k, 1), dtype=torch.int32, device="cuda")
        t_src = torch.empty(max(k, 1), dtype=torch.int32, device="cuda")

        def fill():
            rc = lib.nexg_fragment_frames(ctx, ctypes.byref(fc), ctypes.byref(oc), P(first.data_ptr()), P(nbytes.data_ptr()), k,
                                          P(t_off.data_ptr()), P(t_len.data_ptr()), P(t_src.data_ptr()), P(out.data_ptr()), total, st)
            assert rc == abi.OK

        t = emit("fragment_frames", fill, 200, inner + total + n * 20 + k * 16, case=label, mtu=mtu, output_frames=k,
                 bytes_read=inner, bytes_written=total, table_bytes=n * 20 + k * 16)
        # a spot check against the host contract: the first and last 200 input frames
        torch.cuda.synchronize()
        hf, hr = first.cpu().numpy().view(np.uint32), rows.cpu().numpy().view(abi.FRAGGED_DTYPE)
        hoff, hlen, hsrc = t_off.cpu().numpy(), t_len.cpu().numpy(), t_src.cpu().numpy()
        for j in list(range(min(n, 200))) + list(range(max(0, n - 200), n)):
            fr = batch.data[int(ho[j]): int(ho[j + 1])].cpu().numpy().tobytes()
            want = fragment_frame(fr, mtu)[0]
            assert int(hr["pieces"][j]) == len(want) and int(hr["first"][j]) == int(hf[j]), (label, j)
            for q, w in enumerate(want):
                f = int(hf[j]) + q
                assert int(hsrc[f]) == j and int(hlen[f]) == len(w), (label, j, q)
                assert out[int(hoff[f]): int(hoff[f]) + len(w)].cpu().numpy().tobytes() == w, (label, j, q)
        return t, inner, total

    # every frame under the mtu: a one-to-one copy, beside the gather's and the encapsulation's fills over the same table
    t_pass, inner, _ = measure("IMIX, all pass-through", b, packed.offsets.cpu().numpy(), 9000)
    bc = b.to_c()
    goff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    gwsb = abi.gather_plan_workspace(n)
    gws = torch.empty(gwsb // 8 + 1, dtype=torch.int64, device="cuda")
    assert lib.nexg_gather_plan(ctx, ctypes.byref(bc), 1, P(goff.data_ptr()), None, P(gws.data_ptr()), gwsb, st) == abi.OK
    gtotal = int(goff[n].item())
    dense = torch.empty(max(gtotal, 16), dtype=torch.uint8, device="cuda")

    def gcopy():
        rc = lib.nexg_gather_frames(ctx, ctypes.byref(bc), P(goff.data_ptr()), P(dense.data_ptr()), gtotal, st)
        assert rc == abi.OK

    t_g = emit("gather_frames", gcopy, 200, 2 * gtotal + n * 16, bytes_copied=gtotal)
    del dense
    tunnels = TunnelSet([Tunnel.vxlan(5001, src="10.0.0.1", dst="10.0.0.2", eth_dst="02:00:00:00:00:02",
                                      eth_src="02:00:00:00:00:01", src_port=49152)])
    tc = tunnels.to_c()
    assert lib.nexg_encap_plan(ctx, ctypes.byref(bc), ctypes.byref(tc), None, 1, P(goff.data_ptr()), None, P(gws.data_ptr()), gwsb,
                               st) == abi.OK
    etotal = int(goff[n].item())
    outer = torch.empty(max(etotal, 16), dtype=torch.uint8, device="cuda")

    def efill():
        rc = lib.nexg_encap_frames(ctx, ctypes.byref(bc), ctypes.byref(tc), None, None, P(goff.data_ptr()), P(outer.data_ptr()), etotal,
                                   None, st)
        assert rc == abi.OK

    t_e = emit("encap_frames vxlan4", efill, 200, inner + etotal + n * 16, bytes_read=inner, bytes_written=etotal)
    print(json.dumps({"what": "time ratios, all pass-through", "fragment_frames / gather_frames": round(t_pass / t_g, 3),
                      "fragment_frames / encap_frames": round(t_pass / t_e, 3)}), flush=True)

    # the encapsulated batch on a 1500-byte link: a packed batch as it stands
    from nex_amd.engine import FrameBatch
    torch.cuda.synchronize()
    enc = FrameBatch(data=outer[:etotal], count=n, offsets=goff)
    t_split, _, _ = measure("IMIX behind VXLAN, the 1500-byte class splits", enc, goff.cpu().numpy(), 1500)
    print(json.dumps({"what": "time ratio, fragment_frames split / pass-through", "ratio": round(t_split / t_pass, 3)}), flush=True)


if __name__ == "__main__":
    main()
