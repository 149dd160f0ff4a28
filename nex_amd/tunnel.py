"""Host side of tunnel decapsulation (include/nexg.h nexg_decap_batch).

VxlanHeader / GreHeader carry the reference's field names
(nex-packet/src/vxlan.rs:17-23, gre.rs:11-27); tunnel_view builds one from a
nexg_tunnel plus the outer frame's bytes; decap_host restates the semantics of
nexg_decap_batch for one frame in plain Python (the expectation the device
output is tested against).
"""
from dataclasses import dataclass, field
from typing import List, Optional, Union

from . import abi


@dataclass
class VxlanHeader:
    """VxlanPacket without its payload (vxlan.rs:17-23)."""
    flags: int = 0
    reserved1: int = 0  # u24be
    vni: int = 0        # u24be
    reserved2: int = 0

    def to_bytes(self) -> bytes:
        """VxlanPacket::header (vxlan.rs:85-95)."""
        return (bytes([self.flags]) + self.reserved1.to_bytes(3, "big") + self.vni.to_bytes(3, "big") +
                bytes([self.reserved2]))


@dataclass
class GreHeader:
    """GrePacket without its payload (gre.rs:11-27); the Vec fields are lists
    of 0 or 1 items (`routing` is always empty: the reference does not parse
    source-routed GRE)."""
    checksum_present: int = 0
    routing_present: int = 0
    key_present: int = 0
    sequence_present: int = 0
    strict_source_route: int = 0
    recursion_control: int = 0
    zero_flags: int = 0
    version: int = 0
    protocol_type: int = 0
    checksum: List[int] = field(default_factory=list)
    offset: List[int] = field(default_factory=list)
    key: List[int] = field(default_factory=list)
    sequence: List[int] = field(default_factory=list)
    routing: bytes = b""

    def flags_word(self) -> int:
        return (self.checksum_present << 15 | self.routing_present << 14 | self.key_present << 13 |
                self.sequence_present << 12 | self.strict_source_route << 11 | self.recursion_control << 8 |
                self.zero_flags << 3 | self.version)

    def to_bytes(self) -> bytes:
        """GrePacket::header (gre.rs:163-208): absent optional fields write nothing."""
        out = self.flags_word().to_bytes(2, "big") + self.protocol_type.to_bytes(2, "big")
        if self.checksum_present or self.routing_present:
            out += b"".join(c.to_bytes(2, "big") for c in self.checksum)
            out += b"".join(o.to_bytes(2, "big") for o in self.offset)
        if self.key_present:
            out += b"".join(k.to_bytes(4, "big") for k in self.key)
        if self.sequence_present:
            out += b"".join(s.to_bytes(4, "big") for s in self.sequence)
        if self.routing_present:
            out += bytes(self.routing)
        return out

    def header_len(self) -> int:
        """gre.rs:214-221."""
        cr = self.checksum_present | self.routing_present
        return 4 + 4 * cr + 4 * self.key_present + 4 * self.sequence_present + \
            (len(self.routing) if self.routing_present else 0)


def _tun(kind=abi.TUN_NONE, status=abi.FRAME_OK, inner=abi.INNER_OTHER, hdr_len=0, flags=0, proto=0, id=0, aux=0):
    return {"kind": kind, "status": status, "inner": inner, "hdr_len": hdr_len, "flags": flags, "proto": proto,
            "id": id, "aux": aux}


GRE_INNER = {0x6558: abi.INNER_ETHERNET, 0x0800: abi.INNER_IPV4, 0x86DD: abi.INNER_IPV6}


def vxlan_fields(payload: bytes):
    """VxlanPacket::try_from_buf (vxlan.rs:28-65) as nexg_tunnel fields, or
    None where it returns None."""
    if len(payload) < 8:
        return None
    reserved1 = int.from_bytes(payload[1:4], "big")
    return _tun(abi.TUN_VXLAN, abi.FRAME_OK, abi.INNER_ETHERNET, 8, payload[0], 0,
                int.from_bytes(payload[4:7], "big"), reserved1 << 8 | payload[7])


def gre_fields(payload: bytes):
    """GrePacket::try_from_buf (gre.rs:32-107) as nexg_tunnel fields, or None
    where it returns None: the optional fields are consumed in order, each
    needing 4 bytes, and the routing bit fails after them."""
    if len(payload) < 4:
        return None
    flags = int.from_bytes(payload[0:2], "big")
    proto = int.from_bytes(payload[2:4], "big")
    pos, key, seq = 4, 0, 0
    if flags & 0xC000:  # checksum_present or routing_present: checksum + offset
        if len(payload) - pos < 4:
            return None
        pos += 4
    if flags & 0x2000:
        if len(payload) - pos < 4:
            return None
        key = int.from_bytes(payload[pos:pos + 4], "big")
        pos += 4
    if flags & 0x1000:
        if len(payload) - pos < 4:
            return None
        seq = int.from_bytes(payload[pos:pos + 4], "big")
        pos += 4
    if flags & 0x4000:
        return None
    return _tun(abi.TUN_GRE, abi.FRAME_OK, GRE_INNER.get(proto, abi.INNER_OTHER), pos, flags, proto, key, seq)


def decap_host(frame: bytes, record, which: int = abi.DECAP_VXLAN | abi.DECAP_GRE,
               vxlan_port: int = abi.VXLAN_PORT):
    """nexg_decap_batch for one frame (include/nexg.h): `record` is the frame's
    NEXG_OUT_RECORD record (abi.RECORD_DTYPE element or a mapping). Returns
    (nexg_tunnel fields as a dict, inner offset inside the frame, inner
    length); a frame that is no accepted tunnel gives offset 0, length 0."""
    flags = int(record["flags"])
    poff, plen = int(record["payload_off"]), int(record["payload_len"])
    if (flags >> abi.STATUS_SHIFT) & 7 or poff + plen > len(frame):
        return _tun(), 0, 0
    vxlan_port = vxlan_port or abi.VXLAN_PORT
    payload = bytes(frame[poff:poff + plen])
    if which & abi.DECAP_VXLAN and flags & abi.L_UDP and int(record["dst_port"]) == vxlan_port:
        t, kind = vxlan_fields(payload), abi.TUN_VXLAN
    elif (which & abi.DECAP_GRE and flags & (abi.L_IPV4 | abi.L_IPV6) and
          not flags & (abi.L_TRANSPORT | abi.L_ICMP | abi.L_ICMPV6) and int(record["ip_proto"]) == 47):
        t, kind = gre_fields(payload), abi.TUN_GRE
    else:
        return _tun(), 0, 0
    if t is None:
        return _tun(kind, abi.ERR_MALFORMED), 0, 0
    return t, poff + t["hdr_len"], plen - t["hdr_len"]


def tunnel_view(tun, frame: bytes, record) -> Optional[Union[VxlanHeader, GreHeader]]:
    """The reference's header struct of an accepted tunnel: `tun` a nexg_tunnel
    (abi.TUNNEL_DTYPE element or decap_host's dict), `frame` the outer frame,
    `record` its record. The GRE checksum and offset words are not in
    nexg_tunnel: they are read from the frame at [payload_off + 4,
    payload_off + 8). None for a frame that is no accepted tunnel."""
    kind = int(tun["kind"])
    if kind == abi.TUN_NONE or int(tun["status"]) != abi.FRAME_OK:
        return None
    if kind == abi.TUN_VXLAN:
        aux = int(tun["aux"])
        return VxlanHeader(flags=int(tun["flags"]) & 0xFF, reserved1=aux >> 8, vni=int(tun["id"]), reserved2=aux & 0xFF)
    f = int(tun["flags"])
    h = GreHeader(checksum_present=f >> 15 & 1, routing_present=f >> 14 & 1, key_present=f >> 13 & 1,
                  sequence_present=f >> 12 & 1, strict_source_route=f >> 11 & 1, recursion_control=f >> 8 & 7,
                  zero_flags=f >> 3 & 0x1F, version=f & 7, protocol_type=int(tun["proto"]))
    if h.checksum_present or h.routing_present:
        p = int(record["payload_off"]) + 4
        h.checksum = [int.from_bytes(frame[p:p + 2], "big")]
        h.offset = [int.from_bytes(frame[p + 2:p + 4], "big")]
    if h.key_present:
        h.key = [int(tun["id"])]
    if h.sequence_present:
        h.sequence = [int(tun["aux"])]
    return h
