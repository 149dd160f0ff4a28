"""Batched counterpart of the reference's `examples/dns_dump.rs`: frames from
a capture file are parsed on the GPU a batch at a time (NEXG_OUT_RECORD), every
UDP payload that is not empty is tried as a DNS message (Engine.dns with
any_udp=True, as dns_dump.rs:98-100 does), and for every message that parses
the lines of dns_dump.rs:102-147 are printed: the addresses and ports, each
query's name, type and class, and the answers' addresses (A, AAAA), names
(CNAME, NS, PTR) and TXT strings.

One deviation: a query name that fails to decode prints Err(<ParseError
variant>), e.g. Err(CompressionLoop), where the reference's {:?} also prints
the variant's fields (Err(CompressionLoop { context: "DNS name" })).

    python -m nex_amd.dns_dump capture.pcap [--batch N] [--limit N]
"""
import argparse
import ipaddress
import sys
from typing import Iterator, List

import numpy as np

from . import abi
from .dns import DnsNameError, DnsPacket, frame_entries


def rust_debug_str(s: str) -> str:
    """A string as Rust's {:?} prints it."""
    out = []
    for ch in s:
        if ch in ('"', "\\"):
            out.append("\\" + ch)
        elif ch == "\n":
            out.append("\\n")
        elif ch == "\r":
            out.append("\\r")
        elif ch == "\t":
            out.append("\\t")
        elif ch == "\0":
            out.append("\\0")
        elif not ch.isprintable():
            out.append("\\u{%x}" % ord(ch))
        else:
            out.append(ch)
    return '"' + "".join(out) + '"'


def rust_ip(addr) -> str:
    """An address as Rust's Display prints it (IPv4-mapped IPv6 in dotted form)."""
    if isinstance(addr, ipaddress.IPv6Address) and addr.ipv4_mapped is not None:
        return "::ffff:" + str(addr.ipv4_mapped)
    return str(addr)


def dns_lines(src, sport: int, dst, dport: int, dns: DnsPacket) -> List[str]:
    """dns_dump.rs:102-147 for one parsed message."""
    lines = [f"DNS Packet: {rust_ip(src)}:{sport} > {rust_ip(dst)}:{dport}"]
    for q in dns.queries:
        try:
            name = f"Ok({rust_debug_str(q.qname_parsed())})"
        except DnsNameError as e:
            name = f"Err({e.kind})"
        lines.append(f"  Query: {name} (type: {q.qtype!r}, class: {q.qclass!r})")
    for r in dns.responses:
        t = r.rtype.name
        if t in ("A", "AAAA"):
            ip = r.ip()
            lines.append(f"  Response: {rust_ip(ip)} (type: {r.rtype!r}, ttl: {r.ttl})" if ip is not None
                         else f"  Invalid IP data for type: {r.rtype!r}")
        elif t in ("CNAME", "NS", "PTR"):
            name = r.dns_name()
            lines.append(f"  Response: {name} (type: {r.rtype!r}, ttl: {r.ttl})" if name is not None
                         else f"  Invalid name data for type: {r.rtype!r}")
        elif t == "TXT":
            txts = r.txt_strings()
            if txts is None:
                lines.append("  Invalid TXT data")
            else:
                lines += [f'  TXT: "{x}" (ttl: {r.ttl})' for x in txts]
    return lines


def frame_addresses(frame: bytes, rec):
    """(source, destination) of a parsed UDP frame from its IP header."""
    l3 = int(rec["l3_off"])
    if int(rec["flags"]) & abi.L_IPV4:
        return ipaddress.IPv4Address(frame[l3 + 12:l3 + 16]), ipaddress.IPv4Address(frame[l3 + 16:l3 + 20])
    return ipaddress.IPv6Address(frame[l3 + 8:l3 + 24]), ipaddress.IPv6Address(frame[l3 + 24:l3 + 40])


def dump_batch(frames, recs, dns, tile_first, entries) -> Iterator[str]:
    """The lines of every message of one batch that parsed (host arrays)."""
    for i in np.nonzero((dns["status"] == 0) & (dns["flags8"] & abi.DNS_CANDIDATE != 0))[0]:
        i = int(i)
        src, dst = frame_addresses(frames[i], recs[i])
        pkt = DnsPacket(frames[i], dns[i], frame_entries(dns, tile_first, entries, i))
        yield from dns_lines(src, int(recs[i]["src_port"]), dst, int(recs[i]["dst_port"]), pkt)


def dump_capture(path: str, engine=None, batch_frames: int = 1 << 16, limit: int = 0) -> Iterator[str]:
    import torch

    from .engine import Engine, FrameBatch
    from .ingest import PcapReader
    eng = engine or Engine(0)
    rd = PcapReader(path)
    data = np.empty(batch_frames * 2048, np.uint8)
    offs = np.empty(batch_frames + 1, np.uint64)
    no = 1
    while True:
        n = rd.read_into(data, offs)
        if n == 0:
            break
        if limit:
            n = min(n, limit - no + 1)
        end = int(offs[n])
        frames = [bytes(data[int(offs[i]):int(offs[i + 1])]) for i in range(n)]
        dev = torch.from_numpy(data[:max(end, 16)].copy()).to(eng.torch_device)
        doffs = torch.from_numpy(offs[:n + 1].astype(np.int64)).to(eng.torch_device)
        batch = FrameBatch(data=dev, count=n, offsets=doffs)
        recs = eng.parse(batch, out_kind=abi.OUT_RECORD)
        dns, tile_first, entries, _ = eng.dns(batch, recs, any_udp=True)
        torch.cuda.synchronize(eng.torch_device)
        yield from dump_batch(frames, recs.cpu().numpy()[: n * 64].view(abi.RECORD_DTYPE),
                              dns.cpu().numpy().view(abi.DNS_DTYPE), tile_first.cpu().numpy(),
                              entries.cpu().numpy().view(abi.DNS_ENTRY_DTYPE))
        no += n
        if limit and no > limit:
            break


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("capture", help="pcap / pcapng file")
    ap.add_argument("--batch", type=int, default=1 << 16, help="frames per GPU batch")
    ap.add_argument("--limit", type=int, default=0, help="stop after N frames")
    args = ap.parse_args(argv)
    for line in dump_capture(args.capture, batch_frames=args.batch, limit=args.limit):
        print(line)


if __name__ == "__main__":
    sys.exit(main())
