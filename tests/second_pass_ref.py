"""Independent references for the four second passes (DNS, decap, select,
flow), written in the shape of the reference's parsers and of the text of
include/nexg.h, not in the shape of the kernels or of nex_amd's host contracts.

DNS / GRE / VXLAN consume a memoryview that is re-sliced as the Rust re-slices
`buf` (dns.rs:752-790, 904-945, 1166-1259; gre.rs:32-107; vxlan.rs:28-65) and
return objects with the reference's field names, or the error; separate small
functions map those objects to nexg_dns / nexg_dns_entry / nexg_tunnel fields,
recovering offsets as len(message) - len(remaining). The Toeplitz hash is a
shift register over the key as one integer, prefixes go through the standard
library's ipaddress networks, the partition is numpy's stable argsort.

tests/test_second_pass_ref.py pins these by the reference's own asserted
vectors (tests/golden) and compares nex_amd's contracts with them on the fuzz
corpus; tests/test_gpu_second_pass_fuzz.py compares the kernels with them."""
import functools
import ipaddress
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from nex_amd import abi


# ---- a &[u8] that is re-sliced ---------------------------------------------------------

class Buf:
    """`&mut &[u8]`: every read re-slices the view, as bytes::Buf does."""

    def __init__(self, data):
        self.b = memoryview(bytes(data))

    def remaining(self) -> int:
        return len(self.b)

    def get_u8(self) -> int:
        v = self.b[0]
        self.b = self.b[1:]
        return v

    def get_u16(self) -> int:
        v = int.from_bytes(self.b[:2], "big")
        self.b = self.b[2:]
        return v

    def get_u32(self) -> int:
        v = int.from_bytes(self.b[:4], "big")
        self.b = self.b[4:]
        return v

    def take(self, n: int) -> bytes:
        v = bytes(self.b[:n])
        self.b = self.b[n:]
        return v


# ---- DNS ---------------------------------------------------------------------------------

@dataclass
class DnsQueryRef:  # DnsQueryPacket
    qname: bytes
    qtype: int
    qclass: int
    payload: bytes  # everything after the query


@dataclass
class DnsResponseRef:  # DnsResponsePacket
    name_tag: int
    rtype: int
    rclass: int
    ttl: int
    data_len: int
    data: bytes
    payload: bytes  # everything after the record


@dataclass
class DnsHeaderRef:
    id: int
    is_response: int
    opcode: int
    is_authoriative: int
    is_truncated: int
    is_recursion_desirable: int
    is_recursion_available: int
    zero_reserved: int
    is_answer_authenticated: int
    is_non_authenticated_data: int
    rcode: int
    query_count: int
    response_count: int
    authority_rr_count: int
    additional_rr_count: int


@dataclass
class DnsPacketRef:
    header: DnsHeaderRef
    queries: List[DnsQueryRef]
    responses: List[DnsResponseRef]
    authorities: List[DnsResponseRef]
    additionals: List[DnsResponseRef]
    payload: bytes


@dataclass
class DnsErrorRef:
    kind: str      # "BufferTooShort" | "Malformed"
    context: str


def dns_query_from_buf(buf: Buf) -> Optional[DnsQueryRef]:
    """DnsQueryPacket::from_buf_mut, dns.rs:752-790."""
    qname = bytearray()
    while True:
        if buf.remaining() == 0:
            return None
        ln = buf.get_u8()
        qname.append(ln)
        if ln == 0:
            break
        if buf.remaining() < ln:
            return None
        qname += buf.take(ln)
    if buf.remaining() < 4:
        return None
    qtype = buf.get_u16()
    qclass = buf.get_u16()
    return DnsQueryRef(bytes(qname), qtype, qclass, bytes(buf.b))


def dns_response_from_buf(buf: Buf) -> Optional[DnsResponseRef]:
    """DnsResponsePacket::from_buf_mut, dns.rs:904-945."""
    if buf.remaining() < 12:
        return None
    name_tag = buf.get_u16()
    rtype = buf.get_u16()
    rclass = buf.get_u16()
    ttl = buf.get_u32()
    data_len = buf.get_u16()
    safe_data_len = min(buf.remaining(), data_len)
    data = buf.take(safe_data_len)
    return DnsResponseRef(name_tag, rtype, rclass, ttl, data_len, data, bytes(buf.b))


def dns_try_from_buf(message):
    """DnsPacket::try_from_buf, dns.rs:1166-1259: a DnsPacketRef or a DnsErrorRef."""
    if len(message) < 12:
        return DnsErrorRef("BufferTooShort", "DNS packet")
    cursor = Buf(message)
    ident = cursor.get_u16()
    flags = cursor.get_u16()
    query_count = cursor.get_u16()
    response_count = cursor.get_u16()
    authority_rr_count = cursor.get_u16()
    additional_rr_count = cursor.get_u16()
    header = DnsHeaderRef(ident, flags >> 15 & 1, flags >> 11 & 0xF, flags >> 10 & 1, flags >> 9 & 1, flags >> 8 & 1,
                          flags >> 7 & 1, flags >> 6 & 1, flags >> 5 & 1, flags >> 4 & 1, flags & 0xF, query_count,
                          response_count, authority_rr_count, additional_rr_count)

    def parse_queries(count):
        out = []
        for _ in range(count):
            q = dns_query_from_buf(cursor)
            if q is None:
                return None
            out.append(q)
        return out

    def parse_responses(count):
        out = []
        for _ in range(count):
            r = dns_response_from_buf(cursor)
            if r is None:
                break
            out.append(r)
        return out

    queries = parse_queries(query_count)
    if queries is None:
        return DnsErrorRef("Malformed", "DNS query section")
    responses = parse_responses(response_count)
    authorities = parse_responses(authority_rr_count)
    additionals = parse_responses(additional_rr_count)
    return DnsPacketRef(header, queries, responses, authorities, additionals, bytes(cursor.b))


DNS_SUMMARY_FIELDS = ("status", "flags8", "msg_len", "id", "flags", "qd", "an", "ns", "ar", "n_q", "n_an", "n_ns", "n_ar",
                      "rest_off")


def dns_rows(message, parsed=None):
    """nexg_dns summary fields (but msg_off and first) and nexg_dns_entry rows
    of a message, from the objects dns_try_from_buf returns."""
    message = bytes(message)
    n = len(message)
    p = dns_try_from_buf(message) if parsed is None else parsed
    s = dict.fromkeys(DNS_SUMMARY_FIELDS, 0)
    if isinstance(p, DnsErrorRef) and p.kind == "BufferTooShort":
        s["status"] = abi.ERR_BUFFER_TOO_SHORT
        return s, []
    words = [int.from_bytes(message[2 * k:2 * k + 2], "big") for k in range(6)]
    s.update(flags8=abi.DNS_CANDIDATE, msg_len=n, id=words[0], flags=words[1], qd=words[2], an=words[3], ns=words[4],
             ar=words[5])
    if isinstance(p, DnsErrorRef):
        s["status"] = abi.ERR_MALFORMED
        return s, []
    rows = []
    for q in p.queries:
        size = len(q.qname) + 4
        rows.append(dict(section=abi.DNS_QUERY, flags8=0, off=n - len(q.payload) - size, type=q.qtype, dns_class=q.qclass,
                         ttl=0, name=len(q.qname), data_len=0))
    short = False
    for section, lst, declared in ((abi.DNS_ANSWER, p.responses, p.header.response_count),
                                   (abi.DNS_AUTHORITY, p.authorities, p.header.authority_rr_count),
                                   (abi.DNS_ADDITIONAL, p.additionals, p.header.additional_rr_count)):
        short = short or len(lst) < declared
        for r in lst:
            size = 12 + len(r.data)
            rows.append(dict(section=section, flags8=abi.DNS_DATA_CUT if len(r.data) < r.data_len else 0,
                             off=n - len(r.payload) - size, type=r.rtype, dns_class=r.rclass, ttl=r.ttl, name=r.name_tag,
                             data_len=r.data_len))
    s.update(n_q=len(p.queries), n_an=len(p.responses), n_ns=len(p.authorities), n_ar=len(p.additionals),
             rest_off=n - len(p.payload))
    if short:
        s["flags8"] |= abi.DNS_SECTION_SHORT
    return s, rows


def first_short_section(message) -> int:
    """1, 2 or 3: the first record section with fewer records than declared
    (0: none, or no parsed message)."""
    p = dns_try_from_buf(bytes(message))
    if isinstance(p, DnsErrorRef):
        return 0
    for k, (lst, declared) in enumerate(((p.responses, p.header.response_count),
                                         (p.authorities, p.header.authority_rr_count),
                                         (p.additionals, p.header.additional_rr_count)), 1):
        if len(lst) < declared:
            return k
    return 0


def qname_label_ends_message(message) -> bool:
    """Some label of a declared query takes the message's last byte (no
    terminator follows it): the state in which `buf.len() < len` is an equality."""
    if len(message) < 12:
        return False
    b = Buf(message)
    b.take(4)
    count = b.get_u16()
    b.take(6)
    for _ in range(count):
        while True:
            if b.remaining() == 0:
                return False
            ln = b.get_u8()
            if ln == 0:
                break
            if b.remaining() < ln:
                return False
            b.take(ln)
            if b.remaining() == 0:
                return True
        if b.remaining() < 4:
            return False
        b.take(4)
    return False


def _status(rec) -> int:
    return int(rec["flags"]) >> abi.STATUS_SHIFT & 7


def udp_payload(frame, rec) -> Optional[bytes]:
    """Frame.payload of a frame whose record has status 0 and a UDP layer, the
    payload not empty and inside the frame; else None."""
    poff, plen = int(rec["payload_off"]), int(rec["payload_len"])
    if _status(rec) != 0 or not int(rec["flags"]) & abi.L_UDP or plen == 0 or poff + plen > len(frame):
        return None
    return bytes(frame[poff:poff + plen])


def dns_frame_rows(frame, rec, port=abi.DNS_PORT, any_udp=False):
    """nexg_dns_batch / nexg_dns_entries for one frame: (summary with msg_off, rows)."""
    none = dict(dict.fromkeys(DNS_SUMMARY_FIELDS, 0), msg_off=0), []
    msg = udp_payload(frame, rec)
    if msg is None:
        return none
    if not any_udp and (port or abi.DNS_PORT) not in (int(rec["src_port"]), int(rec["dst_port"])):
        return none
    s, rows = dns_rows(msg)
    s["msg_off"] = int(rec["payload_off"]) if s["flags8"] & abi.DNS_CANDIDATE else 0
    return s, rows


# ---- GRE and VXLAN --------------------------------------------------------------------------

@dataclass
class GreRef:  # GrePacket
    checksum_present: int
    routing_present: int
    key_present: int
    sequence_present: int
    strict_source_route: int
    recursion_control: int
    zero_flags: int
    version: int
    protocol_type: int
    checksum: List[int] = field(default_factory=list)
    offset: List[int] = field(default_factory=list)
    key: List[int] = field(default_factory=list)
    sequence: List[int] = field(default_factory=list)
    routing: bytes = b""
    payload: bytes = b""


@dataclass
class VxlanRef:  # VxlanPacket
    flags: int
    reserved1: int
    vni: int
    reserved2: int
    payload: bytes


def gre_try_from_buf(data) -> Optional[GreRef]:
    """GrePacket::try_from_buf, gre.rs:32-107 (None where it fails)."""
    b = Buf(data)
    if b.remaining() < 4:
        return None
    flags = b.get_u16()
    protocol_type = b.get_u16()
    g = GreRef(flags >> 15 & 1, flags >> 14 & 1, flags >> 13 & 1, flags >> 12 & 1, flags >> 11 & 1, flags >> 8 & 7,
               flags >> 3 & 0x1F, flags & 7, protocol_type)
    if g.checksum_present != 0 or g.routing_present != 0:
        if b.remaining() < 4:
            return None
        g.checksum.append(b.get_u16())
        g.offset.append(b.get_u16())
    if g.key_present != 0:
        if b.remaining() < 4:
            return None
        g.key.append(b.get_u32())
    if g.sequence_present != 0:
        if b.remaining() < 4:
            return None
        g.sequence.append(b.get_u32())
    if g.routing_present != 0:
        return None  # source-routed GRE is not parsed
    g.payload = bytes(b.b)
    return g


def vxlan_try_from_buf(data) -> Optional[VxlanRef]:
    """VxlanPacket::try_from_buf, vxlan.rs:28-65."""
    b = Buf(data)
    if b.remaining() < 8:
        return None
    flags = b.get_u8()
    reserved1 = b.get_u8() << 16 | b.get_u8() << 8 | b.get_u8()
    vni = b.get_u8() << 16 | b.get_u8() << 8 | b.get_u8()
    reserved2 = b.get_u8()
    return VxlanRef(flags, reserved1, vni, reserved2, bytes(b.b))


_NO_TUNNEL = dict(kind=abi.TUN_NONE, status=abi.FRAME_OK, inner=0, hdr_len=0, flags=0, proto=0, id=0, aux=0)
_GRE_CLASS = {0x6558: abi.INNER_ETHERNET, 0x0800: abi.INNER_IPV4, 0x86DD: abi.INNER_IPV6}


def gre_tunnel(data):
    """nexg_tunnel fields of a GRE payload (None where the parser fails)."""
    g = gre_try_from_buf(data)
    if g is None:
        return None
    word = (g.checksum_present << 15 | g.routing_present << 14 | g.key_present << 13 | g.sequence_present << 12 |
            g.strict_source_route << 11 | g.recursion_control << 8 | g.zero_flags << 3 | g.version)
    return dict(kind=abi.TUN_GRE, status=abi.FRAME_OK, inner=_GRE_CLASS.get(g.protocol_type, abi.INNER_OTHER),
                hdr_len=len(data) - len(g.payload), flags=word, proto=g.protocol_type, id=g.key[0] if g.key else 0,
                aux=g.sequence[0] if g.sequence else 0)


def vxlan_tunnel(data):
    v = vxlan_try_from_buf(data)
    if v is None:
        return None
    return dict(kind=abi.TUN_VXLAN, status=abi.FRAME_OK, inner=abi.INNER_ETHERNET, hdr_len=len(data) - len(v.payload),
                flags=v.flags, proto=0, id=v.vni, aux=v.reserved1 << 8 | v.reserved2)


def tunnel_candidate(frame, rec, which=abi.DECAP_VXLAN | abi.DECAP_GRE, vxlan_port=abi.VXLAN_PORT) -> int:
    """abi.TUN_* of the parser nexg_decap_batch tries on the frame (include/nexg.h, "Candidates")."""
    fl = int(rec["flags"])
    if _status(rec) != 0 or int(rec["payload_off"]) + int(rec["payload_len"]) > len(frame):
        return abi.TUN_NONE
    if which & abi.DECAP_VXLAN and fl & abi.L_UDP and int(rec["dst_port"]) == (vxlan_port or abi.VXLAN_PORT):
        return abi.TUN_VXLAN
    layers = abi.L_TRANSPORT | abi.L_ICMP | abi.L_ICMPV6
    if which & abi.DECAP_GRE and fl & (abi.L_IPV4 | abi.L_IPV6) and not fl & layers and int(rec["ip_proto"]) == 47:
        return abi.TUN_GRE
    return abi.TUN_NONE


def decap_frame(frame, rec, which=abi.DECAP_VXLAN | abi.DECAP_GRE, vxlan_port=abi.VXLAN_PORT):
    """nexg_decap_batch for one frame: (nexg_tunnel fields, inner offset inside the frame, inner length)."""
    kind = tunnel_candidate(frame, rec, which, vxlan_port)
    if kind == abi.TUN_NONE:
        return dict(_NO_TUNNEL), 0, 0
    poff, plen = int(rec["payload_off"]), int(rec["payload_len"])
    payload = bytes(frame[poff:poff + plen])
    t = vxlan_tunnel(payload) if kind == abi.TUN_VXLAN else gre_tunnel(payload)
    if t is None:
        return dict(_NO_TUNNEL, kind=kind, status=abi.ERR_MALFORMED), 0, 0
    return t, poff + t["hdr_len"], plen - t["hdr_len"]


# ---- select ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _network(want: bytes, bits: int):
    cls = ipaddress.IPv4Network if len(want) == 4 else ipaddress.IPv6Network
    return cls((want, bits), strict=False)


def in_prefix(addr: bytes, want: bytes, bits: int) -> bool:
    """`addr` lies in the network want/bits, by the standard library."""
    addr = bytes(addr)
    return ipaddress.ip_address(addr) in _network(bytes(want)[:len(addr)], bits)


def frame_addresses(frame, rec, length, family):
    """(src, dst) bytes for an address test of `family`, None when the frame has none (include/nexg.h)."""
    fl = int(rec["flags"])
    if _status(rec) != 0:
        return None
    if family == 4:
        if not fl & abi.L_IPV4:
            return None
        return int(rec["ip_src"]).to_bytes(4, "big"), int(rec["ip_dst"]).to_bytes(4, "big")
    l3 = int(rec["l3_off"])
    if not fl & abi.L_IPV6 or frame is None or length > 65535 or l3 + 40 > length:
        return None
    return bytes(frame[l3 + 8:l3 + 24]), bytes(frame[l3 + 24:l3 + 40])


def rule_verdict(frame, rec, length, r) -> bool:
    """One nexg_rule on one frame, test by test as include/nexg.h lists them."""
    fl = int(rec["flags"])
    verdicts = [fl & r.flags_mask == r.flags_value]
    good = _status(rec) == 0
    has_ports = good and fl & (abi.L_TCP | abi.L_UDP) != 0
    sp, dp = int(rec["src_port"]), int(rec["dst_port"])
    t = r.tests
    if t & abi.RULE_PROTO:
        verdicts.append(good and fl & (abi.L_IPV4 | abi.L_IPV6) != 0 and int(rec["ip_proto"]) == r.ip_proto)
    if t & abi.RULE_SRC_PORT:
        verdicts.append(has_ports and sp in range(r.sport_lo, r.sport_hi + 1))
    if t & abi.RULE_DST_PORT:
        verdicts.append(has_ports and dp in range(r.dport_lo, r.dport_hi + 1))
    if t & abi.RULE_ANY_PORT:
        ports = range(r.sport_lo, r.sport_hi + 1)
        verdicts.append(has_ports and (sp in ports or dp in ports))
    if t & (abi.RULE_SRC_ADDR | abi.RULE_DST_ADDR | abi.RULE_ANY_ADDR):
        a = frame_addresses(frame, rec, length, r.family)
        if a is None:
            verdicts.append(False)
        else:
            if t & abi.RULE_SRC_ADDR:
                verdicts.append(in_prefix(a[0], r.src, r.src_bits))
            if t & abi.RULE_DST_ADDR:
                verdicts.append(in_prefix(a[1], r.dst, r.dst_bits))
            if t & abi.RULE_ANY_ADDR:
                verdicts.append(any(in_prefix(x, r.src, r.src_bits) for x in a))
    if t & abi.RULE_TCP_FLAGS:
        verdicts.append(good and fl & abi.L_TCP != 0 and int(rec["l4_type"]) & r.tcp_mask == r.tcp_value)
    if t & abi.RULE_LENGTH:
        verdicts.append(length in range(r.len_lo, r.len_hi + 1))
    return all(verdicts)


def filter_verdict(frame, rec, length, flt):
    """(selected, out_rule) of nexg_select_batch for one frame."""
    hits = [i for i, r in enumerate(flt.rules) if rule_verdict(frame, rec, length, r)]
    if flt.raw_flags() & abi.FILTER_INVERT:
        return not hits, abi.RULE_NONE
    return bool(hits), hits[0] if hits else abi.RULE_NONE


# ---- flow ------------------------------------------------------------------------------------

def toeplitz_shift(data: bytes, key: bytes) -> int:
    """The Toeplitz hash as a shift register: the key is one integer; for every
    input bit, most significant first, the register's top 32 bits are XORed in
    when the bit is set, then the register moves left by one."""
    nbits = 8 * len(key)
    reg = int.from_bytes(key, "big")
    mask = (1 << nbits) - 1
    h = 0
    for byte in bytes(data):
        for bit in (128, 64, 32, 16, 8, 4, 2, 1):
            if byte & bit:
                h ^= reg >> (nbits - 32)
            reg = (reg << 1) & mask
    return h


def flow_row(frame, rec, length, symmetric=False, ports=True, key=None):
    """nexg_flow_batch's row for one frame: (hash, kind, proto, swapped), from the text of include/nexg.h."""
    from nex_amd.flow import DEFAULT_KEY
    fl = int(rec["flags"])
    a = None
    if fl & abi.L_IPV4:
        a, v6 = frame_addresses(frame, rec, length, 4), False
    elif fl & abi.L_IPV6:
        a, v6 = frame_addresses(frame, rec, length, 6), True
    if a is None:
        return 0, abi.FLOW_NONE, 0, 0
    with_ports = ports and fl & (abi.L_TCP | abi.L_UDP) != 0
    if not v6:
        word = int(rec["ip_word"])
        more_fragments, fragment_offset = word >> 13 & 1, word & 0x1FFF
        if more_fragments or fragment_offset:
            with_ports = False
    src_side, dst_side = [a[0]], [a[1]]
    if with_ports:
        src_side.append(int(rec["src_port"]).to_bytes(2, "big"))
        dst_side.append(int(rec["dst_port"]).to_bytes(2, "big"))
    swapped = 0
    if symmetric and b"".join(src_side) > b"".join(dst_side):
        src_side, dst_side, swapped = dst_side, src_side, 1
    key_bytes = src_side[0] + dst_side[0] + b"".join(src_side[1:]) + b"".join(dst_side[1:])
    kind = {(False, False): abi.FLOW_IPV4, (False, True): abi.FLOW_IPV4_L4, (True, False): abi.FLOW_IPV6,
            (True, True): abi.FLOW_IPV6_L4}[(v6, bool(with_ports))]
    return toeplitz_shift(key_bytes, DEFAULT_KEY if key is None else key), kind, int(rec["ip_proto"]), swapped


def flow_rows(frames, recs, lengths, symmetric=False, ports=True, key=None):
    out = np.zeros(len(frames), abi.FLOW_DTYPE)
    for i, f in enumerate(frames):
        out[i] = flow_row(f, recs[i], int(lengths[i]), symmetric, ports, key) + (0,)
    return out


def partition(hashes, buckets: int):
    """(index, bucket_first) of nexg_flow_partition: the stable argsort of hash % buckets."""
    b = (np.asarray(hashes, np.uint64) % np.uint64(buckets)).astype(np.int64)
    index = np.argsort(b, kind="stable")
    first = np.searchsorted(b[index], np.arange(buckets + 1), side="left").astype(np.int64)
    return index.astype(np.uint32), first
