"""Flow test traffic: a small explicit corpus for nexg_flow_batch /
nexg_flow_partition (include/nexg.h) with, per frame, what its construction
implies for the flow row (kind, whether the ports join the key, the key
bytes), so the expectation does not come from the code under test. The first
frames are the published RSS verification vectors
(tests/golden/flow_vectors.json) as TCP and as UDP frames and their reverse
directions; tests/select_frames.corpus() follows for breadth. The corpus is
parsed with NEXG_PARSE_VLAN | NEXG_PARSE_STRICT, as the selection corpus is."""
import json
import os
from dataclasses import dataclass
from typing import Optional

from nex_amd import abi
from tests import helpers
from tests import select_frames as sf
from tests.helpers import rfc1071
from tests.select_frames import eth, ip, ip4, ip6, tcp_seg, udp_dgram

PARSE_FLAGS = sf.PARSE_FLAGS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def vectors():
    """The golden vectors: dicts with src, sport, dst, dport, hash_l4, hash_ip (ints)."""
    with open(os.path.join(ROOT, "tests", "golden", "flow_vectors.json")) as f:
        doc = json.load(f)
    return [dict(v, hash_l4=int(v["hash_l4"], 16), hash_ip=int(v["hash_ip"], 16)) for v in doc["vectors"]]


@dataclass
class F:
    frame: bytes
    what: str
    kind: Optional[int] = None   # abi.FLOW_* the construction implies (None: no claim, e.g. the selection corpus)
    key: bytes = b""             # the key bytes without NEXG_FLOW_SYMMETRIC
    key_ip: bytes = b""          # ... under NEXG_FLOW_NO_PORTS
    proto: int = 0
    hash_l4: Optional[int] = None  # the golden hashes, where the frame is a vector
    hash_ip: Optional[int] = None
    conv: Optional[str] = None   # frames of one conversation (both directions) share this tag


def ip4_frag(src, dst, proto, payload, mf=False, frag_off=0, ident=0x4321):
    """An IPv4 packet with the given MF bit and fragment offset (8-B units)."""
    tot = 20 + len(payload)
    fo = (0x2000 if mf else 0) | frag_off
    h = (bytes([0x45, 0]) + tot.to_bytes(2, "big") + ident.to_bytes(2, "big") + fo.to_bytes(2, "big") +
         bytes([64, proto]) + bytes(2) + ip(src) + ip(dst))
    return h[:10] + rfc1071(h).to_bytes(2, "big") + h[12:] + payload


def _l4_frame(l4, src, dst, sport, dport, payload=b""):
    seg = tcp_seg(src, dst, sport, dport, 0x10, payload) if l4 == "tcp" else udp_dgram(src, dst, sport, dport, payload)
    proto = 6 if l4 == "tcp" else 17
    if ":" in src:
        return eth(ip6(src, dst, proto, seg), 0x86DD), proto
    return eth(ip4(src, dst, proto, seg)), proto


def _tuple(l4, src, dst, sport, dport, what, payload=b"", **kw):
    fr, proto = _l4_frame(l4, src, dst, sport, dport, payload)
    six = ":" in src
    a = ip(src) + ip(dst)
    return F(fr, what, abi.FLOW_IPV6_L4 if six else abi.FLOW_IPV4_L4, a + sport.to_bytes(2, "big") + dport.to_bytes(2, "big"),
             a, proto, **kw)


A4, B4 = "10.0.0.1", "10.1.2.3"
A6, B6 = "2001:db8::1", "2001:db8:1::2"


def own_corpus():
    """The frames this module builds (every one with a claim about its row)."""
    c = []
    for i, v in enumerate(vectors()):
        for l4 in ("tcp", "udp"):
            c.append(_tuple(l4, v["src"], v["dst"], v["sport"], v["dport"], f"vector {i} {l4}", hash_l4=v["hash_l4"],
                            hash_ip=v["hash_ip"], conv=f"v{i}{l4}"))
            c.append(_tuple(l4, v["dst"], v["src"], v["dport"], v["sport"], f"vector {i} {l4} reversed", conv=f"v{i}{l4}"))
    # one 5-tuple, two payloads
    c.append(_tuple("udp", A4, B4, 1111, 2222, "5-tuple payload 1", b"one", conv="pay"))
    c.append(_tuple("udp", A4, B4, 1111, 2222, "5-tuple payload 2", b"another payload", conv="pay"))
    # equal addresses: under SYMMETRIC the ports decide; equal endpoints: never swapped
    c.append(_tuple("udp", A4, A4, 9, 7, "same address, ports 9 -> 7", conv="same"))
    c.append(_tuple("udp", A4, A4, 7, 9, "same address, ports 7 -> 9", conv="same"))
    c.append(_tuple("tcp", A6, A6, 5, 5, "same endpoint"))
    # fragments of a UDP datagram: the first (MF, carries the UDP header) and a later one
    dgram = udp_dgram(A4, B4, 3333, 4444, bytes(range(48)))
    a = ip(A4) + ip(B4)
    c.append(F(eth(ip4_frag(A4, B4, 17, dgram[:24], mf=True)), "v4 first fragment (MF)", abi.FLOW_IPV4, a, a, 17, conv="frag"))
    c.append(F(eth(ip4_frag(A4, B4, 17, dgram[24:], frag_off=3)), "v4 later fragment (offset 3)", abi.FLOW_IPV4, a, a, 17,
               conv="frag"))
    c.append(F(eth(ip4_frag(A4, B4, 17, dgram[24:48], mf=True, frag_off=3)), "v4 middle fragment (MF, offset 3)",
               abi.FLOW_IPV4, a, a, 17, conv="frag"))
    # ICMP, ICMPv6, a protocol the parser gives no L4 layer
    c.append(F(eth(ip4(A4, B4, 1, sf.icmp_echo())), "v4 icmp", abi.FLOW_IPV4, a, a, 1))
    a6 = ip(A6) + ip(B6)
    c.append(F(eth(ip6(A6, B6, 58, sf.icmpv6_echo(A6, B6)), 0x86DD), "v6 icmpv6", abi.FLOW_IPV6, a6, a6, 58))
    c.append(F(eth(ip4(A4, B4, 132, bytes(16))), "v4 sctp (no L4 layer)", abi.FLOW_IPV4, a, a, 132))
    c.append(F(eth(ip6(A6, B6, 132, bytes(16)), 0x86DD), "v6 sctp (no L4 layer)", abi.FLOW_IPV6, a6, a6, 132))
    # no flow
    arp = bytes([0, 1, 8, 0, 6, 4, 0, 1]) + bytes(range(6)) + ip(A4) + bytes(6) + ip(B4)
    c.append(F(eth(arp, 0x0806), "arp", abi.FLOW_NONE))
    c.append(F(eth(bytes(32), 0x88CC), "unknown ethertype", abi.FLOW_NONE))
    c.append(F(helpers.crafted_frames()[9], "ipv4 total > captured (error status)", abi.FLOW_NONE))
    c.append(F(eth(ip6(A6, B6, 17, udp_dgram(A6, B6, 1, 2)), 0x86DD)[: 14 + 8 + 20], "v6 cut inside the addresses",
               abi.FLOW_NONE))
    # VLAN-tagged, parsed with unwrap_vlan
    t = _tuple("udp", A4, B4, 1111, 2222, "vlan 5-tuple", b"tagged", conv="pay")
    t.frame = helpers.vlan(t.frame, [0x0064])
    c.append(t)
    return c


def corpus():
    """own_corpus() + the selection corpus (no claims: breadth for the GPU-vs-host comparison)."""
    return own_corpus() + [F(x.frame, "select: " + x.what) for x in sf.corpus()]


def small_corpus():
    """The corpus without its 65535-byte frame (for batches tiled to tens of thousands of frames)."""
    return [x for x in corpus() if len(x.frame) < 65535]
