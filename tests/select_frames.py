"""Selection test traffic: a small explicit corpus for nexg_select_batch /
nexg_gather_* (include/nexg.h) with, per frame, the classes its construction
implies (family, L4 kind, ports, addresses, TCP flags, status, checksum
verdicts), so the expectation of what a rule should pick does not come from
the code under test. The corpus is parsed with NEXG_PARSE_VLAN |
NEXG_PARSE_STRICT: strict mode is what makes each ParseError kind appear.

RULES is the table of rules the GPU tests run; tests/test_select_host.py
asserts that each selects some but not all of the corpus."""
import ipaddress
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from nex_amd import abi
from nex_amd.select import TCP_ACK, TCP_FIN, TCP_SYN, Filter, Rule
from tests import helpers
from tests.helpers import rfc1071

PARSE_FLAGS = abi.PARSE_VLAN | abi.PARSE_STRICT
MAC = bytes(range(1, 13))

A4, B4, C4, D4, E4 = "10.0.0.1", "10.1.2.3", "192.168.1.10", "172.16.0.5", "11.0.0.1"
A6, B6, C6 = "2001:db8::1", "2001:db8:1::2", "fe80::1"
X6 = "2001:db8:aaaa:bbbb:cccc:dddd:eeee:ffff"  # the address the prefix-bit frames vary
PREFIX_BITS = (1, 31, 32, 33, 64, 127, 128)


def ip(a) -> bytes:
    return ipaddress.ip_address(a).packed


def flip_bit(addr: str, n: int) -> str:
    """`addr` with its n-th bit from the top (1-based) inverted."""
    b = bytearray(ip(addr))
    b[(n - 1) // 8] ^= 0x80 >> ((n - 1) % 8)
    return str(ipaddress.ip_address(bytes(b)))


def _pseudo(src: bytes, dst: bytes, proto: int, n: int) -> bytes:
    if len(src) == 4:
        return src + dst + bytes([0, proto]) + n.to_bytes(2, "big")
    return src + dst + n.to_bytes(4, "big") + bytes([0, 0, 0, proto])


def tcp_seg(src, dst, sport, dport, flags, payload=b"", opts=b"", bad=False):
    doff = (20 + len(opts)) // 4
    h = (sport.to_bytes(2, "big") + dport.to_bytes(2, "big") + (0x01020304).to_bytes(4, "big") +
         (0x05060708).to_bytes(4, "big") + bytes([doff << 4, flags]) + (0x2000).to_bytes(2, "big"))
    seg = h + bytes(4) + opts + payload
    c = rfc1071(_pseudo(ip(src), ip(dst), 6, len(seg)) + seg) ^ (0x5555 if bad else 0)
    return h + c.to_bytes(2, "big") + bytes(2) + opts + payload


def udp_dgram(src, dst, sport, dport, payload=b"", bad=False):
    n = 8 + len(payload)
    h = sport.to_bytes(2, "big") + dport.to_bytes(2, "big") + n.to_bytes(2, "big")
    c = rfc1071(_pseudo(ip(src), ip(dst), 17, n) + h + bytes(2) + payload) or 0xFFFF
    return h + (c ^ (0x5555 if bad else 0)).to_bytes(2, "big") + payload


def icmp_echo(payload=b"ping"):
    h = bytes([8, 0]) + bytes(2) + bytes([0, 1, 0, 2]) + payload
    return h[:2] + rfc1071(h).to_bytes(2, "big") + h[4:]


def icmpv6_echo(src, dst, payload=b"ping"):
    h = bytes([128, 0]) + bytes(2) + bytes([0, 1, 0, 2]) + payload
    c = rfc1071(_pseudo(ip(src), ip(dst), 58, len(h)) + h)
    return h[:2] + c.to_bytes(2, "big") + h[4:]


def ip4(src, dst, proto, payload, bad=False):
    tot = 20 + len(payload)
    h = bytes([0x45, 0]) + tot.to_bytes(2, "big") + bytes([0x12, 0x34, 0x40, 0, 64, proto]) + bytes(2) + ip(src) + ip(dst)
    c = rfc1071(h) ^ (0x5555 if bad else 0)
    return h[:10] + c.to_bytes(2, "big") + h[12:] + payload


def ip6(src, dst, nh, payload):
    return bytes([0x60, 0, 0, 0]) + len(payload).to_bytes(2, "big") + bytes([nh, 64]) + ip(src) + ip(dst) + payload


def eth(p, et=0x0800):
    return MAC + et.to_bytes(2, "big") + p


@dataclass
class F:
    frame: bytes
    what: str
    fam: int = 0             # 4 / 6 when the frame parses to that IP layer
    l4: Optional[str] = None  # "tcp" | "udp" | "icmp" | "icmpv6"
    src: Optional[str] = None
    dst: Optional[str] = None
    sport: int = 0
    dport: int = 0
    tcp_flags: int = 0
    status: int = 0
    bad_ip: bool = False
    bad_l4: bool = False
    arp: bool = False
    vlan: bool = False
    junk: bool = False       # a mutated frame: no class is claimed for it
    cls: dict = field(default_factory=dict)


def _v4(l4, src, dst, sport, dport, what, tcp_flags=0, payload=b"", opts=b"", bad_ip=False, bad_l4=False, pad_to=0):
    seg = (tcp_seg(src, dst, sport, dport, tcp_flags, payload, opts, bad_l4) if l4 == "tcp"
           else udp_dgram(src, dst, sport, dport, payload, bad_l4))
    fr = eth(ip4(src, dst, 6 if l4 == "tcp" else 17, seg, bad_ip))
    fr += bytes(max(0, pad_to - len(fr)))
    return F(fr, what, 4, l4, src, dst, sport, dport, tcp_flags, bad_ip=bad_ip, bad_l4=bad_l4)


def _v6(l4, src, dst, sport, dport, what, tcp_flags=0, payload=b"", opts=b"", hbh=False):
    seg = (tcp_seg(src, dst, sport, dport, tcp_flags, payload, opts) if l4 == "tcp"
           else udp_dgram(src, dst, sport, dport, payload))
    proto = 6 if l4 == "tcp" else 17
    body = ip6(src, dst, 0, bytes([proto, 0]) + bytes(6) + seg) if hbh else ip6(src, dst, proto, seg)
    if hbh:  # the reference dispatches on the fixed header's next header (0): no transport layer behind an extension
        return F(eth(body, 0x86DD), what, 6, None, src, dst)
    return F(eth(body, 0x86DD), what, 6, l4, src, dst, sport, dport, tcp_flags)


SYN_OPTS = b"\x02\x04\x05\xb4\x04\x02\x08\x0a" + bytes(8) + b"\x01\x03\x03\x07"


def corpus():
    """About 60 frames; see the module docstring."""
    P = bytes(range(32))
    c = []
    # IPv4 x TCP / UDP / ICMP
    c.append(_v4("tcp", A4, B4, 40000, 80, "v4 tcp syn", TCP_SYN))
    c.append(_v4("tcp", B4, A4, 80, 40000, "v4 tcp syn|ack", TCP_SYN | TCP_ACK))
    c.append(_v4("tcp", A4, C4, 40001, 443, "v4 tcp fin|ack", TCP_FIN | TCP_ACK, P))
    c.append(_v4("tcp", C4, A4, 50000, 22, "v4 tcp syn with options", TCP_SYN, opts=SYN_OPTS))
    c.append(_v4("udp", A4, B4, 33333, 53, "v4 udp to 53", payload=P))
    c.append(_v4("udp", C4, D4, 5353, 5353, "v4 udp mdns", payload=P[:9]))
    c.append(_v4("udp", D4, A4, 44444, 4789, "v4 udp to 4789", payload=P))
    c.append(_v4("udp", B4, C4, 50001, 50002, "v4 udp ephemeral", payload=P[:1]))
    c.append(_v4("udp", E4, D4, 53, 33000, "v4 udp from 53, 11/8", payload=P))
    c.append(_v4("udp", "0.0.0.0", "255.255.255.255", 68, 67, "v4 udp dhcp discover from 0.0.0.0", payload=P))
    c.append(F(eth(ip4(A4, D4, 1, icmp_echo())), "v4 icmp echo", 4, "icmp", A4, D4))
    # IPv6 x TCP / UDP / ICMPv6
    c.append(_v6("tcp", A6, B6, 40000, 80, "v6 tcp syn", TCP_SYN))
    c.append(_v6("tcp", B6, A6, 80, 40000, "v6 tcp syn|ack", TCP_SYN | TCP_ACK))
    c.append(_v6("tcp", A6, C6, 40001, 443, "v6 tcp fin", TCP_FIN, P))
    c.append(_v6("tcp", C6, A6, 50000, 22, "v6 tcp syn with options", TCP_SYN, opts=SYN_OPTS))
    c.append(_v6("udp", A6, B6, 33333, 53, "v6 udp to 53", payload=P))
    c.append(_v6("udp", C6, C6, 5353, 5353, "v6 udp mdns", payload=P[:9]))
    c.append(_v6("udp", B6, A6, 44444, 4789, "v6 udp to 4789", payload=P))
    c.append(_v6("udp", B6, C6, 50001, 50002, "v6 udp ephemeral", payload=P[:1]))
    c.append(F(eth(ip6(A6, B6, 58, icmpv6_echo(A6, B6)), 0x86DD), "v6 icmpv6 echo", 6, "icmpv6", A6, B6))
    c.append(_v6("udp", A6, B6, 33334, 53, "v6 hop-by-hop + udp", payload=P, hbh=True))
    # addresses that differ from X6 at one prefix bit
    c.append(_v6("udp", X6, B6, 1000, 2000, "v6 src X"))
    for n in PREFIX_BITS:
        c.append(_v6("udp", flip_bit(X6, n), B6, 1000, 2000, f"v6 src X bit {n}"))
    for n in (33, 64):
        c.append(_v6("udp", B6, flip_bit(X6, n), 1000, 2000, f"v6 dst X bit {n}"))
    # ARP, VLAN, unknown EtherType
    arp = bytes([0, 1, 8, 0, 6, 4, 0, 1]) + bytes(range(6)) + ip(A4) + bytes(6) + ip(B4)
    c.append(F(eth(arp, 0x0806), "arp request", arp=True))
    c.append(F(helpers.vlan(_v4("udp", A4, B4, 33335, 53, "", payload=P).frame, [0x0064]), "vlan v4 udp to 53", 4, "udp",
               A4, B4, 33335, 53, vlan=True))
    c.append(F(eth(P, 0x88CC), "lldp (unknown ethertype)"))
    # checksum failures
    c.append(_v4("udp", A4, B4, 33336, 9999, "v4 udp bad ip checksum", payload=P, bad_ip=True))
    c.append(_v4("tcp", A4, B4, 40002, 8080, "v4 tcp bad l4 checksum", TCP_ACK, P, bad_l4=True))
    # each ParseError kind (strict parse); their records carry the error's payload
    cf = helpers.crafted_frames()
    c.append(F(bytes(13), "13 bytes", status=abi.ERR_BUFFER_TOO_SHORT))
    c.append(F(cf[5], "ipv4 ihl < 5", status=abi.ERR_INVALID_LENGTH))
    c.append(F(cf[4], "ipv4 version 5", status=abi.ERR_MALFORMED))
    c.append(F(cf[9], "ipv4 total > captured", status=abi.ERR_TRUNCATED))
    # frame lengths 14, 60, 64, 65, 1514, 65535
    c.append(F(eth(b"", 0x1234), "14 bytes"))
    c.append(_v4("udp", A4, B4, 2001, 2002, "60 bytes (padded)", payload=b"x", pad_to=60))
    c.append(_v4("udp", A4, B4, 2001, 2002, "64 bytes (padded)", payload=b"xy", pad_to=64))
    c.append(_v4("udp", A4, B4, 2001, 2002, "65 bytes", payload=bytes(65 - 42)))
    c.append(_v4("udp", D4, C4, 2001, 2002, "1514 bytes", payload=bytes(range(256)) * 5 + bytes(1514 - 42 - 1280)))
    c.append(_v4("udp", D4, C4, 2001, 2002, "65535 bytes", payload=(bytes(range(251)) * 262)[: 65535 - 42]))
    assert [len(x.frame) for x in c[-6:]] == [14, 60, 64, 65, 1514, 65535]
    # junk-field cases
    rng = np.random.default_rng(20260)
    base = [x.frame for x in c if len(x.frame) < 200]
    for i, fr in enumerate(helpers.mutate_frames(rng, base, 12)):
        c.append(F(fr, f"mutated {i}", junk=True))
    return c


def small_corpus():
    """The corpus without its 65535-byte frame (for batches tiled to tens of
    thousands of frames)."""
    return [x for x in corpus() if len(x.frame) < 65535]


def cycled(items, count):
    return [items[i % len(items)] for i in range(count)]


def expected_flags(x: F) -> Optional[int]:
    """The layer / verdict bits the frame's construction implies (None for a
    mutated frame)."""
    if x.junk:
        return None
    if x.status:
        return x.status << abi.STATUS_SHIFT
    fl = abi.L_ETHERNET | (abi.L_VLAN if x.vlan else 0)
    if x.arp:
        return fl | abi.L_ARP
    if not x.fam:
        return fl
    fl |= abi.L_IP | (abi.L_IPV4 | abi.C_IP_CHECKED | (0 if x.bad_ip else abi.C_IP_OK) if x.fam == 4 else abi.L_IPV6)
    if x.l4 is None:
        return fl
    fl |= {"tcp": abi.L_TRANSPORT | abi.L_TCP, "udp": abi.L_TRANSPORT | abi.L_UDP, "icmp": abi.L_ICMP,
           "icmpv6": abi.L_ICMPV6}[x.l4]
    return fl | abi.C_L4_CHECKED | (0 if x.bad_l4 else abi.C_L4_OK)


def _prefix_rules():
    return [(f"v6 src X/{n}", Rule.net(f"{X6}/{n}", "src")) for n in PREFIX_BITS]


#: name -> one rule; every one selects some but not all of the corpus
RULES = dict([
    ("tcp", Rule.tcp()),
    ("udp", Rule.udp()),
    ("tcp syn only", Rule.tcp(syn=True, ack=False)),
    ("tcp syn|ack", Rule.tcp(syn=True, ack=True)),
    ("tcp fin", Rule.tcp(fin=True)),
    ("proto 17", Rule.proto(17)),
    ("proto 58", Rule.proto(58)),
    ("proto 1", Rule.proto(1)),
    ("port 53 any", Rule.port(53)),
    ("port 5353 any", Rule.port(5353)),
    ("dst port 4789", Rule.port(4789, direction="dst")),
    ("src ports 40000-50000", Rule.port(40000, 50000, "src")),
    ("arp junk ports", Rule.port(1, 2048)),          # ARP's hardware / protocol type sit in the port fields
    ("dst net 10/8", Rule.net("10.0.0.0/8", "dst")),
    ("src net 10/8", Rule.net("10.0.0.0/8", "src")),
    ("any net 10.0.0.0/31", Rule.net("10.0.0.0/31")),
    ("host 192.168.1.10", Rule.host(C4)),
    ("v4 /0", Rule.net("0.0.0.0/0", "src")),
    ("junk net 0/8", Rule.net("0.0.0.0/8")),          # an error record's ip_src / ip_dst hold small numbers
    ("src net 2001:db8::/32", Rule.net("2001:db8::/32", "src")),
    ("any host fe80::1", Rule.host(C6)),
    ("dst 2001:db8:1::/48", Rule.net("2001:db8:1::/48", "dst")),
    ("v6 /0", Rule.net("::/0", "dst")),
    ("v6 dst X/33", Rule.net(f"{X6}/33", "dst")),
    ("bad l4 checksum", Rule.bad_checksum("l4")),
    ("bad ip checksum", Rule.bad_checksum("ip")),
    ("status truncated", Rule.status(abi.ERR_TRUNCATED)),
    ("status ok", Rule.status(0)),
    ("vlan", Rule.flags(abi.L_VLAN)),
    ("arp", Rule.flags(abi.L_ARP)),
    ("length 60-65", Rule.length(60, 65)),
    ("length 1514", Rule.length(1514)),
    ("length 0-14", Rule.length(0, 14)),
    ("tcp syn to 10/8", Rule.tcp(syn=True, ack=False) & Rule.net("10.0.0.0/8", "dst")),
    ("udp 53 short", Rule.udp() & Rule.port(53) & Rule.length(0, 100)),
    ("v6 udp from db8", Rule.udp() & Rule.net("2001:db8::/32", "src") & Rule.port(53, direction="dst")),
] + _prefix_rules())

#: multi-rule filters (first-match order matters for out_rule)
FILTERS = {
    "issue examples": Filter([Rule.tcp(syn=True, ack=False) & Rule.net("10.0.0.0/8", "dst"),
                              Rule.udp() & Rule.port(53), Rule.udp() & Rule.port(5353), Rule.bad_checksum("l4"),
                              Rule.net("2001:db8::/32", "src")]),
    "overlapping": Filter([Rule.port(80), Rule.udp(), Rule.proto(6), Rule.status(0)]),
    "sixteen": Filter([Rule.port(p) for p in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 22)] +
                      [Rule.net(f"{X6}/64", "src"), Rule.tcp()]),
    "inverted": Filter([Rule.udp(), Rule.flags(abi.L_ARP)], invert=True),
    "inverted v6": Filter([Rule.net("2001:db8::/32")], invert=True),
    "match all": Filter([Rule.any()]),
    "match none": Filter([Rule.any()], invert=True),
}


def all_filters():
    """(name, Filter) for every table rule alone and every multi-rule filter."""
    return [(n, Filter([r])) for n, r in RULES.items()] + list(FILTERS.items())
