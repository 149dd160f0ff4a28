#!/usr/bin/env python3
"""Rate of tunnel encapsulation on IMIX traffic: nexg_encap_plan and
nexg_encap_frames for VXLAN over IPv4 without and with the outer UDP checksum
and for GRE over IPv4 with key and sequence, at 100 % and near 1 % selection,
beside Engine.gather's two calls (nexg_gather_plan, nexg_gather_frames) over
the same table and a device-to-device copy of as many bytes as the
encapsulation writes (torch copy_ in the same process: the ceiling a copy
kernel is judged against).

The batch and the timing are those of tools/select_rate.py: --frames (default
4M) IMIX frames from Engine.gen_batch, packed, with a u32 offset table; the
tables are the match-all selection and the destination-port range 0-1047
(near 1 %) from nexg_select_batch. Times are HIP events around `steps`
back-to-back calls after warm-up calls, repeated --repeats times (all repeats
are printed; the rates use the fastest). Bytes per call, algorithmic: the plan
reads the table (12 B per frame) twice and writes 12 B per frame (offset and
length); the fill reads the inner bytes once and writes the outer bytes, and
reads the table, the two planned offsets and writes the 8-B row (36 B per
frame). Rates are given as a fraction of 8 TB/s. One JSON line per measurement.

usage: python tools/encap_rate.py [--frames N] [--repeats R] [--quick]
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

    import torch
    from nex_amd import abi
    from nex_amd.encap import Tunnel, TunnelSet, encap_frame
    from nex_amd.engine import Engine
    from nex_amd.select import Filter, Rule
    if not torch.cuda.is_available():
        sys.exit("encap_rate needs the GPU: no rate is reported without one")
    eng = Engine(0)
    stream = torch.cuda.current_stream()
    b = eng.gen_batch(abi.WL_IMIX, args.frames).with_offsets32()
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

    recs = eng.parse(b, out_kind=abi.OUT_RECORD)
    ends = dict(src="10.0.0.1", dst="10.0.0.2", eth_dst="02:00:00:00:00:02", eth_src="02:00:00:00:00:01")
    specs = (("vxlan4", TunnelSet([Tunnel.vxlan(5001, src_port=49152, **ends)])),
             ("vxlan4 + UDP_CSUM", TunnelSet([Tunnel.vxlan(5001, src_port=49152, udp_csum=True, **ends)])),
             ("gre4 key + sequence", TunnelSet([Tunnel.gre(key=7, seq_base=0, **ends)])))
    for fname, rules in (("match all (100 %)", [Rule.any()]), ("dst port 0-1047 (~1 %)", [Rule.port(0, 1047, "dst")])):
        idx, sel = eng.select(b, recs, Filter(rules))
        k = sel.count
        sc = sel.to_c()
        inner = int(sel.lengths.sum().item())
        goff = torch.empty(k + 1, dtype=torch.int64, device="cuda")
        glen = torch.empty(max(k, 1), dtype=torch.int32, device="cuda")
        rows = torch.empty(max(k, 1) * 8, dtype=torch.uint8, device="cuda")
        wsb = abi.encap_plan_workspace(k)
        ws = torch.empty(wsb // 8 + 1, dtype=torch.int64, device="cuda")
        times = {}
        for sname, tunnels in specs:
            tc = tunnels.to_c()

            def plan():
                rc = lib.nexg_encap_plan(ctx, ctypes.byref(sc), ctypes.byref(tc), None, 1, P(goff.data_ptr()), P(glen.data_ptr()),
                                         P(ws.data_ptr()), wsb, st)
                assert rc == abi.OK

            plan()
            total = int(goff[k].item())
            emit("encap_plan", plan, 50, k * (2 * 12 + 12), filter=fname, spec=sname, selected=k)
            outer = torch.empty(max(total, 16), dtype=torch.uint8, device="cuda")

            def fill():
                rc = lib.nexg_encap_frames(ctx, ctypes.byref(sc), ctypes.byref(tc), None, None, P(goff.data_ptr()),
                                           P(outer.data_ptr()), total, P(rows.data_ptr()), st)
                assert rc == abi.OK

            times[sname] = emit("encap_frames", fill, 20, inner + total + k * 36, filter=fname, spec=sname, selected=k,
                                bytes_read=inner, bytes_written=total)
            # a spot check against the host contract: the first and last 200 frames
            torch.cuda.synchronize()
            ho, hl = sel.offsets[:k].cpu().numpy(), sel.lengths[:k].cpu().numpy()
            hg = goff[: k + 1].cpu().numpy()
            for j in list(range(min(k, 200))) + list(range(max(0, k - 200), k)):
                fr = b.data[int(ho[j]): int(ho[j]) + int(hl[j])].cpu().numpy().tobytes()
                want = encap_frame(fr, tunnels.tunnels[0], j)[0]
                assert outer[int(hg[j]): int(hg[j + 1])].cpu().numpy().tobytes() == want, (sname, j)
        print(json.dumps({"what": "encap_frames time ratio, UDP_CSUM / none", "filter": fname,
                          "ratio": round(times["vxlan4 + UDP_CSUM"] / times["vxlan4"], 3)}), flush=True)

        # Engine.gather's two calls over the same table, and a device copy of as many bytes as vxlan4 writes
        def gplan():
            rc = lib.nexg_gather_plan(ctx, ctypes.byref(sc), 1, P(goff.data_ptr()), None, P(ws.data_ptr()), wsb, st)
            assert rc == abi.OK

        gplan()
        gtotal = int(goff[k].item())
        emit("gather_plan", gplan, 50, k * (2 * 12 + 8), filter=fname, selected=k)
        dense = torch.empty(max(gtotal, 16), dtype=torch.uint8, device="cuda")

        def gcopy():
            rc = lib.nexg_gather_frames(ctx, ctypes.byref(sc), P(goff.data_ptr()), P(dense.data_ptr()), gtotal, st)
            assert rc == abi.OK

        t_g = emit("gather_frames", gcopy, 20, 2 * gtotal + k * 20, filter=fname, selected=k, bytes_copied=gtotal)
        m = max(inner + 50 * k, 16)
        src = torch.empty(m, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        t_d = emit("device-to-device copy_ of as many bytes as vxlan4 writes", lambda: dst.copy_(src), 20, 2 * m, filter=fname)
        print(json.dumps({"what": "time ratios", "filter": fname,
                          "encap_frames vxlan4 / copy_": round(times["vxlan4"] / t_d, 3),
                          "encap_frames vxlan4 / gather_frames": round(times["vxlan4"] / t_g, 3),
                          "gather_frames / copy_": round(t_g / t_d, 3)}), flush=True)
        del outer, dense, src, dst


if __name__ == "__main__":
    main()
