#!/usr/bin/env python3
"""Rate of the DNS message pass on synthetic DNS traffic: nexg_dns_batch
(k_dns_walk + the tile scan) and nexg_dns_entries (k_dns_fill), beside the
NEXG_OUT_RECORD parse of the same batch.

The batch: --frames (default 4M) Eth/IPv4/UDP frames at a fixed 96-B stride
with a lengths array, alternating a 38-B query for a seeded name
(qNNNNNNN.example.com, type A) to port 53 and its 54-B one-answer response
from port 53 (frames of 80 and 96 bytes), built on the host from --distinct
pairs and tiled. Times are HIP events around `steps` back-to-back calls after
`warmup` calls, repeated --repeats times (all repeats are printed; the rates
use the fastest). The two kernels of nexg_dns_batch run back to back in one
call: the events time the call, and a second row times the same call on a
batch of empty frames with as many tiles (the record read, the summary store
and the scan, no message byte: the floor under the walk); the kernels' own
durations come from a kernel trace of this program (profiles/dns/). Bytes per
frame, algorithmic: the walk reads 32 B of the record (two 16-B quarters) and
the message (46 B on average) and writes the 32-B summary; the fill reads the
summary and the message again and writes 16 B per entry (1.5 entries per
frame). Rates are given as a fraction of 8 TB/s. One JSON line per
measurement.

usage: python tools/dns_rate.py [--frames N] [--distinct N] [--repeats R] [--quick]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STRIDE = 96
QUERY, RESPONSE = 38, 54  # message bytes


def ipv4_udp(payload_len, sport, dport):
    total = 20 + 8 + payload_len
    ip = bytearray([0x45, 0, total >> 8, total & 255, 0, 0, 0x40, 0, 64, 17, 0, 0, 10, 0, 0, 1, 10, 0, 0, 2])
    s = sum(int.from_bytes(ip[i:i + 2], "big") for i in range(0, 20, 2))
    s = (s & 0xFFFF) + (s >> 16)
    ip[10:12] = (~((s & 0xFFFF) + (s >> 16)) & 0xFFFF).to_bytes(2, "big")
    udp = sport.to_bytes(2, "big") + dport.to_bytes(2, "big") + (8 + payload_len).to_bytes(2, "big") + b"\0\0"
    return bytes(range(1, 13)) + b"\x08\x00" + bytes(ip) + udp


def dns_batch(frames, distinct, seed):
    """Fixed-stride device batch of `frames` frames: query, response, query, ..."""
    import torch
    from nex_amd.engine import FrameBatch
    rng = np.random.default_rng(seed)
    pairs = (distinct + 1) // 2
    a = np.zeros((pairs, 2, STRIDE), np.uint8)
    ids = rng.integers(0, 1 << 16, pairs)
    digits = rng.integers(0, 10, (pairs, 7)).astype(np.uint8) + ord("0")
    tail = b"\x07example\x03com\x00\x00\x01\x00\x01"
    for k, (hdr, flags, an) in enumerate(((ipv4_udp(QUERY, 0xC001, 53), 0x0100, 0),
                                          (ipv4_udp(RESPONSE, 53, 0xC001), 0x8180, 1))):
        a[:, k, :42] = np.frombuffer(hdr, np.uint8)
        a[:, k, 42], a[:, k, 43] = ids >> 8, ids & 255
        a[:, k, 44:54] = np.frombuffer(flags.to_bytes(2, "big") + b"\x00\x01" + an.to_bytes(2, "big") + bytes(4), np.uint8)
        a[:, k, 54], a[:, k, 55] = 8, ord("q")
        a[:, k, 56:63] = digits
        a[:, k, 63:63 + len(tail)] = np.frombuffer(tail, np.uint8)
    assert 63 + len(tail) == 42 + QUERY
    answer = b"\xc0\x0c\x00\x01\x00\x01\x00\x00\x01\x2c\x00\x04"
    a[:, 1, 80:92] = np.frombuffer(answer, np.uint8)
    a[:, 1, 92:96] = rng.integers(1, 255, (pairs, 4))
    flat = torch.from_numpy(a.reshape(-1)).cuda()
    reps = (frames + 2 * pairs - 1) // (2 * pairs)
    data = flat.repeat(reps)[: frames * STRIDE].contiguous()
    lens = torch.tensor([42 + QUERY, 42 + RESPONSE], dtype=torch.int32, device="cuda").repeat((frames + 1) // 2)[:frames]
    return FrameBatch(data=data, count=frames, stride=STRIDE, lengths=lens.contiguous())


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
    ap.add_argument("--seed", type=int, default=53)
    ap.add_argument("--quick", action="store_true",
                    help="2 steps after 1 warm-up call, one repeat: the launches for a counter pass, not a timing")
    args = ap.parse_args()
    import ctypes

    import torch
    from nex_amd import abi
    from nex_amd.engine import Engine, FrameBatch
    if not torch.cuda.is_available():
        sys.exit("dns_rate needs the GPU: no rate is reported without one")
    eng = Engine(0)
    stream = torch.cuda.current_stream()
    b = dns_batch(args.frames, args.distinct, args.seed)
    n = b.count
    recs = torch.empty(n * 64, dtype=torch.uint8, device="cuda")

    def parse_outer():
        eng.parse(b, out_kind=abi.OUT_RECORD, out=recs, stream=stream)

    parse_outer()
    dns, tile_first, entries, total = eng.dns(b, recs, stream=stream)
    torch.cuda.synchronize()
    d = dns.cpu().numpy().view(abi.DNS_DTYPE)
    e = entries.cpu().numpy().view(abi.DNS_ENTRY_DTYPE)
    assert (d["status"] == 0).all() and (d["n_q"] == 1).all() and (d["n_an"] == np.arange(n) % 2).all(), "not every message parsed"
    assert total == n + n // 2 == len(e) and (e["type"] == 1).all() and (d["rest_off"] == d["msg_len"]).all()
    msg = int(d["msg_len"].astype(np.int64).sum())
    del d, e

    # the C calls themselves, on buffers allocated once
    P = ctypes.c_void_p
    fr = b.to_c()
    st = ctypes.c_void_p(stream.cuda_stream)
    lib, ctx = eng.lib, eng.ctx

    def walk_scan():
        rc = lib.nexg_dns_batch(ctx, ctypes.byref(fr), P(recs.data_ptr()), None, P(dns.data_ptr()), P(tile_first.data_ptr()), st)
        assert rc == abi.OK

    def fill():
        rc = lib.nexg_dns_entries(ctx, ctypes.byref(fr), P(dns.data_ptr()), P(tile_first.data_ptr()), P(entries.data_ptr()),
                                  total, st)
        assert rc == abi.OK

    # the scan kernel's share: the same number of tiles over frames of length 0 (every record a non-candidate)
    zero = FrameBatch(data=b.data, count=n, stride=STRIDE, lengths=torch.zeros(n, dtype=torch.int32, device="cuda"))
    zrecs = eng.parse(zero, out_kind=abi.OUT_RECORD, stream=stream)
    zdns = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    ztf = torch.empty_like(tile_first)
    zfr = zero.to_c()

    def scan_tiles():
        rc = lib.nexg_dns_batch(ctx, ctypes.byref(zfr), P(zrecs.data_ptr()), None, P(zdns.data_ptr()), P(ztf.data_ptr()), st)
        assert rc == abi.OK

    rows = (("outer_record_parse", parse_outer, 50, b.total_bytes + n * 64),
            ("dns_batch (k_dns_walk + scan)", walk_scan, 100, n * (32 + 32) + msg),
            ("dns_batch on empty frames (record read + summary store + scan)", scan_tiles, 100, n * (32 + 32)),
            ("dns_entries (k_dns_fill)", fill, 100, n * 32 + msg + total * 16))
    for name, fn, steps, nbytes in rows:
        if args.quick:
            ts = timed(fn, stream, 1, 2, 1)
            steps = 2
        else:
            ts = timed(fn, stream, 5, steps, args.repeats)
        best = min(ts)
        print(json.dumps({"what": name, "frames": n, "entries": total, "steps": steps,
                          "ms": [round(x * 1e3, 4) for x in ts], "bytes_per_call": nbytes,
                          "tb_s": round(nbytes / best / 1e12, 4), "frac_of_8tb_s": round(nbytes / best / 8e12, 4),
                          "mpkt_s": round(n / best / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
