#!/usr/bin/env python3
"""Rate of tunnel decapsulation on VXLAN traffic: k_decap alone, then the whole
chain record parse -> decap -> select -> inner parse, beside the
NEXG_OUT_RECORD parse of the same outer batch (the step that dominates).

The batch: --frames (default 4M) VXLAN frames at a fixed 114-B stride, each a
50-B outer header (Ethernet, IPv4, UDP to 4789, VXLAN) around one 64-B UDP
frame of the headline workload (NEXG_WL_UDP64), built on the host from
--distinct generated frames and tiled. Times are HIP events around `steps`
back-to-back calls after `warmup` calls, repeated --repeats times (all
repeats are printed; the rates use the fastest). k_decap's own bytes per frame
are 64 (record) + 16 (header read) + 28 (written); its rate is given as a
fraction of 8 TB/s. The chain's rate is outer frame bytes per second; it
includes decap_select's read-back of the selected count (one synchronisation
per call). One JSON line per measurement.

usage: python tools/decap_rate.py [--frames N] [--distinct N] [--repeats R]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUTER = 50
INNER = 64


def vxlan_batch(eng, frames, distinct):
    """Fixed-stride device batch of `frames` VXLAN frames (distinct ones tiled)."""
    import torch
    from nex_amd import abi
    from nex_amd.engine import FrameBatch
    inner = eng.gen_batch(abi.WL_UDP64, distinct).data.cpu().numpy().reshape(distinct, INNER)
    total = OUTER - 14 + INNER
    ip = bytearray([0x45, 0, total >> 8, total & 255, 0, 0, 0x40, 0, 64, 17, 0, 0, 10, 0, 0, 1, 10, 0, 0, 2])
    s = sum(int.from_bytes(ip[i:i + 2], "big") for i in range(0, 20, 2))
    s = (s & 0xFFFF) + (s >> 16)
    ip[10:12] = (~((s & 0xFFFF) + (s >> 16)) & 0xFFFF).to_bytes(2, "big")
    ulen = 8 + 8 + INNER
    udp = bytes([0xC0, 0x01]) + (4789).to_bytes(2, "big") + ulen.to_bytes(2, "big") + b"\0\0"
    head = bytes(range(1, 13)) + b"\x08\x00" + bytes(ip) + udp + bytes([0x08, 0, 0, 0])
    a = np.zeros((distinct, OUTER + INNER), np.uint8)
    a[:, :OUTER - 4] = np.frombuffer(head, np.uint8)
    vni = np.arange(distinct, dtype=np.uint32) & 0xFFFFFF
    a[:, OUTER - 4], a[:, OUTER - 3], a[:, OUTER - 2] = vni >> 16, (vni >> 8) & 255, vni & 255
    a[:, OUTER:] = inner
    reps = (frames + distinct - 1) // distinct
    data = torch.from_numpy(a.reshape(-1)).cuda().repeat(reps)[: frames * (OUTER + INNER)].contiguous()
    pad = torch.zeros(16, dtype=torch.uint8, device="cuda")
    data = torch.cat([data, pad])[: frames * (OUTER + INNER)]
    return FrameBatch(data=data, count=frames, stride=OUTER + INNER)


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
    ap.add_argument("--distinct", type=int, default=1 << 16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--quick", action="store_true",
                    help="2 steps after 1 warm-up call, one repeat: the launches for a counter pass, not a timing")
    args = ap.parse_args()
    import torch
    from nex_amd import abi
    from nex_amd.engine import Engine
    from nex_amd.frame import ParseOption
    if not torch.cuda.is_available():
        sys.exit("decap_rate needs the GPU: no rate is reported without one")
    eng = Engine(0)
    stream = torch.cuda.current_stream()
    b = vxlan_batch(eng, args.frames, args.distinct)
    n, fbytes = b.count, b.count * (OUTER + INNER)
    recs = torch.empty(n * 64, dtype=torch.uint8, device="cuda")

    def parse_outer():
        eng.parse(b, out_kind=abi.OUT_RECORD, out=recs, stream=stream)

    parse_outer()
    tunnels, inner = eng.decap(b, recs, stream=stream)
    idx, sel = eng.decap_select(tunnels, inner, {abi.INNER_ETHERNET}, stream=stream)
    t = tunnels.cpu().numpy().view(abi.TUNNEL_DTYPE)
    assert sel.count == n and (t["kind"] == abi.TUN_VXLAN).all() and (t["status"] == 0).all(), "not every frame decapsulated"
    inner_recs = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
    eng.parse(sel, out_kind=abi.OUT_RECORD, out=inner_recs, stream=stream)
    torch.cuda.synchronize()
    ir = inner_recs.cpu().numpy().view(abi.RECORD_DTYPE)
    assert ((ir["flags"] & abi.L_UDP) != 0).all() and (ir["payload_len"] == INNER - 42).all(), "inner parse"
    del t, ir

    def chain():
        parse_outer()
        tu, inn = eng.decap(b, recs, stream=stream)
        _, s = eng.decap_select(tu, inn, {abi.INNER_ETHERNET}, stream=stream)
        eng.parse(s, ParseOption(), out_kind=abi.OUT_RECORD, out=inner_recs, stream=stream)

    rows = (("outer_record_parse", parse_outer, 50, fbytes),
            ("k_decap", lambda: eng.decap(b, recs, stream=stream), 200, n * (64 + 16 + 28)),
            ("inner_record_parse", lambda: eng.parse(sel, out_kind=abi.OUT_RECORD, out=inner_recs, stream=stream), 50,
             n * INNER),
            ("chain", chain, 20, fbytes))
    for name, fn, steps, nbytes in rows:
        if args.quick:
            ts = timed(fn, stream, 1, 2, 1)
            steps = 2
        else:
            ts = timed(fn, stream, 5, steps, args.repeats)
        best = min(ts)
        print(json.dumps({"what": name, "frames": n, "steps": steps, "ms": [round(x * 1e3, 4) for x in ts],
                          "bytes_per_call": nbytes, "tb_s": round(nbytes / best / 1e12, 4),
                          "frac_of_8tb_s": round(nbytes / best / 8e12, 4), "mpkt_s": round(n / best / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
