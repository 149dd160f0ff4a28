"""Host side of tunnel encapsulation (include/nexg.h nexg_encap_plan /
nexg_encap_frames): frames wrapped in an outer Ethernet / IPv4 or IPv6 / UDP +
VXLAN or GRE header, the bytes the reference's builders give when composed as
examples/udp_ping.rs composes them. The other direction of nex_amd.tunnel, and
a match-action table's second action half: rule j of a filter gets tunnel j.

Tunnel and TunnelSet build the C structs and validate exactly as the C entry
does (ValueError where nexg_tunnels_check returns NEXG_EINVAL). encap_host
restates the contract of include/nexg.h in plain Python, one frame at a time,
and is what the device output is tested against (tests/test_encap_host.py pins
it by an independent reference built on the oracle's builders).

    vtep = Tunnel.vxlan(vni=5001, src="10.0.0.1", dst="10.0.0.2", eth_dst="02:00:00:00:00:02",
                        eth_src="02:00:00:00:00:01", src_port=49152, port_span=16384, udp_csum=True)
    gre = Tunnel.gre(src="2001:db8::1", dst="2001:db8::2", key=7, l3=True)
    tunnels = TunnelSet([vtep, gre])
"""
import ipaddress
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import abi
from .tunnel import GreHeader, VxlanHeader


def _mac(v) -> bytes:
    if isinstance(v, str):
        v = bytes(int(x, 16) for x in v.split(":"))
    v = bytes(v)
    if len(v) != 6:
        raise ValueError("tunnel: a MAC address has 6 bytes")
    return v


def _ip(v):
    """(family, 16 bytes) of an address given as text, 4 / 16 bytes or an ipaddress object."""
    if isinstance(v, (str, ipaddress.IPv4Address, ipaddress.IPv6Address)):
        v = ipaddress.ip_address(v).packed
    v = bytes(v)
    if len(v) not in (4, 16):
        raise ValueError("tunnel: an address has 4 or 16 bytes")
    return (4 if len(v) == 4 else 6), v.ljust(16, b"\0")


@dataclass(frozen=True)
class Tunnel:
    """struct nexg_tunnel_spec."""
    kind: int = abi.ENCAP_VXLAN
    family: int = 4
    ttl: int = 64
    tos: int = 0
    flags: int = 0
    eth_dst: bytes = bytes(6)
    eth_src: bytes = bytes(6)
    src: bytes = bytes(16)        # network order; family 4 uses the first 4 bytes
    dst: bytes = bytes(16)
    src_port: int = 0
    dst_port: int = 0             # 0 means 4789
    port_span: int = 0
    ip_id: int = 0
    id: int = 0                   # VXLAN vni / GRE key
    seq_base: int = 0
    flow_label: int = 0
    ip_flags: int = 0
    reserved: bytes = bytes(23)   # raw nexg_tunnel_spec.reserved

    @staticmethod
    def _outer(src, dst):
        (fs, s), (fd, d) = _ip(src), _ip(dst)
        if fs != fd:
            raise ValueError("tunnel: endpoints of different address families")
        return fs, s, d

    @classmethod
    def vxlan(cls, vni, src, dst, eth_dst=bytes(6), eth_src=bytes(6), src_port=0, dst_port=0, port_span=0,
              udp_csum=False, ttl=64, tos=0, ip_id=0, ip_flags=0, flow_label=0) -> "Tunnel":
        """Eth / IP / UDP / VxlanPacket (vxlan.rs:73-84). port_span > 0: the
        source port is src_port + flow hash % port_span (RFC 7348's entropy;
        Engine.encap then needs the rows of Engine.flow)."""
        family, s, d = cls._outer(src, dst)
        flags = (abi.ENCAP_UDP_CSUM if udp_csum else 0) | (abi.ENCAP_FLOW_PORT if port_span else 0)
        return cls(abi.ENCAP_VXLAN, family, ttl, tos, flags, _mac(eth_dst), _mac(eth_src), s, d, src_port, dst_port,
                   port_span, ip_id, vni, 0, flow_label, ip_flags)

    @classmethod
    def gre(cls, src, dst, eth_dst=bytes(6), eth_src=bytes(6), key=None, seq_base=None, l3=False, ttl=64, tos=0,
            ip_id=0, ip_flags=0, flow_label=0) -> "Tunnel":
        """Eth / IP (protocol 47) / GrePacket (gre.rs:115-160). key: the K bit
        and the key; seq_base: the S bit, frame i gets seq_base + i; l3: the
        inner Ethernet header is dropped and its EtherType becomes the
        protocol type."""
        family, s, d = cls._outer(src, dst)
        flags = ((abi.ENCAP_GRE_KEY if key is not None else 0) | (abi.ENCAP_GRE_SEQ if seq_base is not None else 0) |
                 (abi.ENCAP_GRE_L3 if l3 else 0))
        return cls(abi.ENCAP_GRE, family, ttl, tos, flags, _mac(eth_dst), _mac(eth_src), s, d, 0, 0, 0, ip_id, key or 0,
                   seq_base or 0, flow_label, ip_flags)

    # ---- the C form ----------------------------------------------------------
    def validate(self) -> "Tunnel":
        """ValueError for what nexg_tunnels_check rejects (and for a value a field cannot hold)."""
        if self.kind not in (abi.ENCAP_VXLAN, abi.ENCAP_GRE):
            raise ValueError("tunnel: kind must be VXLAN or GRE")
        if self.family not in (4, 6):
            raise ValueError("tunnel: family must be 4 or 6")
        if not 0 <= self.flags <= 0xFFFFFFFF or self.flags & ~(abi.ENCAP_VXLAN_FLAGS | abi.ENCAP_GRE_FLAGS):
            raise ValueError("tunnel: unknown flag bits")
        if self.kind == abi.ENCAP_VXLAN and self.flags & abi.ENCAP_GRE_FLAGS:
            raise ValueError("tunnel: a GRE flag on a VXLAN spec")
        if self.kind == abi.ENCAP_GRE and self.flags & abi.ENCAP_VXLAN_FLAGS:
            raise ValueError("tunnel: a VXLAN flag on a GRE spec")
        if not 0 <= self.id <= (0xFFFFFF if self.kind == abi.ENCAP_VXLAN else 0xFFFFFFFF):
            raise ValueError("tunnel: a VXLAN id has 24 bits, a GRE key 32")
        if not 0 <= self.flow_label <= 0xFFFFF:
            raise ValueError("tunnel: flow_label has 20 bits")
        if not 0 <= self.ip_flags <= 7:
            raise ValueError("tunnel: ip_flags has 3 bits")
        for name, top in (("ttl", 0xFF), ("tos", 0xFF), ("src_port", 0xFFFF), ("dst_port", 0xFFFF), ("port_span", 0xFFFF),
                          ("ip_id", 0xFFFF), ("seq_base", 0xFFFFFFFF)):
            if not 0 <= getattr(self, name) <= top:
                raise ValueError(f"tunnel: {name} out of range")
        if self.flags & abi.ENCAP_FLOW_PORT:
            if self.port_span == 0 or self.src_port + self.port_span > 65536:
                raise ValueError("tunnel: FLOW_PORT needs 1 <= port_span <= 65536 - src_port")
        elif self.port_span:
            raise ValueError("tunnel: port_span without FLOW_PORT")
        if any(bytes(self.reserved)):
            raise ValueError("tunnel: reserved must be 0")
        return self

    def to_c(self, check=True) -> abi.TunnelSpecC:
        if check:
            self.validate()
        c = abi.TunnelSpecC(kind=self.kind, family=self.family, ttl=self.ttl, tos=self.tos, flags=self.flags,
                            src_port=self.src_port, dst_port=self.dst_port, port_span=self.port_span, ip_id=self.ip_id,
                            id=self.id, seq_base=self.seq_base, flow_label=self.flow_label, ip_flags=self.ip_flags)
        for name, n in (("eth_dst", 6), ("eth_src", 6), ("src", 16), ("dst", 16), ("reserved", 23)):
            getattr(c, name)[:] = list(bytes(getattr(self, name)).ljust(n, b"\0")[:n])
        return c

    # ---- what the header is made of --------------------------------------------
    @property
    def l3_mode(self) -> bool:
        return bool(self.flags & abi.ENCAP_GRE_L3)

    def header_len(self) -> int:
        """H of include/nexg.h."""
        ip = 20 if self.family == 4 else 40
        if self.kind == abi.ENCAP_VXLAN:
            return 14 + ip + 16
        return 14 + ip + 4 + 4 * bool(self.flags & abi.ENCAP_GRE_KEY) + 4 * bool(self.flags & abi.ENCAP_GRE_SEQ)


@dataclass(frozen=True)
class TunnelSet:
    """struct nexg_tunnels: 1..16 specs."""
    tunnels: Sequence[Tunnel]
    reserved: int = 0

    def validate(self) -> "TunnelSet":
        if not 1 <= len(self.tunnels) <= abi.ENCAP_MAX_TUNNELS:
            raise ValueError("tunnel set: 1..16 tunnels")
        if self.reserved:
            raise ValueError("tunnel set: reserved must be 0")
        for t in self.tunnels:
            t.validate()
        return self

    def to_c(self, check=True) -> abi.TunnelsC:
        if check:
            self.validate()
        c = abi.TunnelsC(n_tunnels=len(self.tunnels), reserved=self.reserved)
        for i, t in enumerate(self.tunnels[: abi.ENCAP_MAX_TUNNELS]):
            c.tunnels[i] = t.to_c(check)
        return c

    @property
    def needs_flows(self) -> bool:
        return any(t.flags & abi.ENCAP_FLOW_PORT for t in self.tunnels)


def _sum16(data: bytes) -> int:
    """Sum of the big-endian 16-bit words of `data`, an odd last byte padded with 0 (util.rs:169-183)."""
    if len(data) % 2:
        data += b"\0"
    return sum(int.from_bytes(data[i:i + 2], "big") for i in range(0, len(data), 2))


def _finalize(s: int) -> int:
    """util.rs:73-78."""
    while s >> 16:
        s = (s >> 16) + (s & 0xFFFF)
    return ~s & 0xFFFF


def _row(status=abi.FRAME_OK, tunnel=abi.TUNNEL_NONE, hdr_len=0, src_port=0, l4_csum=0):
    return (status, tunnel, hdr_len, 0, src_port, l4_csum)


def encap_frame(frame: Optional[bytes], t: Optional[Tunnel], index: int = 0, flow_hash: int = 0, tunnel: int = 0):
    """Rules 1-4 of include/nexg.h for one frame: (outer bytes, nexg_encapped
    as a tuple). `frame` None: an extent the table does not hold; `t` None: a
    pass-through; `tunnel`: the frame's tunnel_index value, for the row."""
    if frame is None:
        return b"", _row(abi.ERR_BAD_EXTENT, tunnel)
    frame = bytes(frame)
    if t is None:
        return frame, _row()
    proto_type = 0x6558
    payload = frame
    if t.l3_mode:
        if len(frame) < 14:
            return b"", _row(abi.ERR_BUFFER_TOO_SHORT, tunnel)
        proto_type = int.from_bytes(frame[12:14], "big")
        payload = frame[14:]
    H, m = t.header_len(), len(payload)
    if H + m > 65535:
        return b"", _row(abi.ERR_INVALID_LENGTH, tunnel)
    v4 = t.family == 4
    src, dst = (t.src[:4], t.dst[:4]) if v4 else (t.src, t.dst)
    ip_proto = 17 if t.kind == abi.ENCAP_VXLAN else 47
    port = csum = 0
    if t.kind == abi.ENCAP_VXLAN:
        port = t.src_port + (flow_hash % t.port_span if t.flags & abi.ENCAP_FLOW_PORT else 0)
        body = VxlanHeader(flags=0x08, vni=t.id).to_bytes() + payload
        udp = port.to_bytes(2, "big") + (t.dst_port or abi.VXLAN_PORT).to_bytes(2, "big") + (8 + len(body)).to_bytes(2, "big")
        if t.flags & abi.ENCAP_UDP_CSUM:  # udp::checksum: pseudo-header, then the datagram with the field as 0
            csum = _finalize(_sum16(src) + _sum16(dst) + 17 + 8 + len(body) + _sum16(udp + b"\0\0" + body))
        l4 = udp + csum.to_bytes(2, "big") + body
    else:
        K, S = bool(t.flags & abi.ENCAP_GRE_KEY), bool(t.flags & abi.ENCAP_GRE_SEQ)
        l4 = GreHeader(key_present=int(K), sequence_present=int(S), protocol_type=proto_type, key=[t.id] if K else [],
                       sequence=[(t.seq_base + index) & 0xFFFFFFFF] if S else []).to_bytes() + payload
    if v4:
        ip = (bytes([0x45, t.tos]) + (20 + len(l4)).to_bytes(2, "big") + t.ip_id.to_bytes(2, "big") +
              bytes([t.ip_flags << 5, 0, t.ttl, ip_proto]))
        ip += _finalize(_sum16(ip + src + dst)).to_bytes(2, "big") + src + dst
    else:
        ip = (bytes([0x60 | t.tos >> 4, (t.tos & 15) << 4 | t.flow_label >> 16, t.flow_label >> 8 & 0xFF,
                     t.flow_label & 0xFF]) + len(l4).to_bytes(2, "big") + bytes([ip_proto, t.ttl]) + src + dst)
    out = t.eth_dst + t.eth_src + (b"\x08\x00" if v4 else b"\x86\xdd") + ip + l4
    assert len(out) == H + m
    return out, _row(abi.FRAME_OK, tunnel, H, port, csum)


def encap_host(frames: Sequence[Optional[bytes]], tunnels: TunnelSet, index=None, flows=None):
    """nexg_encap_plan + nexg_encap_frames in plain Python: (outer frames, rows
    as an abi.ENCAPPED_DTYPE array). `frames`: bytes, or None for an extent
    outside the data; `index`: one tunnel number per frame or None (tunnel 0
    for all); `flows`: an abi.FLOW_DTYPE array (or a sequence of hash values)
    when a spec has FLOW_PORT."""
    tunnels.validate()
    if tunnels.needs_flows and flows is None:
        raise ValueError("encap: a spec has FLOW_PORT and flows is None")
    specs: List[Tunnel] = list(tunnels.tunnels)
    out, rows = [], np.zeros(len(frames), abi.ENCAPPED_DTYPE)
    for i, f in enumerate(frames):
        n = 0 if index is None else int(index[i])
        h = 0
        if flows is not None:
            h = int(flows[i]["hash"]) if getattr(flows, "dtype", None) is not None and flows.dtype.names else int(flows[i])
        b, row = encap_frame(f, specs[n] if n < len(specs) else None, i, h, n)
        out.append(b)
        rows[i] = row
    return out, rows


def plan_host(lengths: Sequence[int], align: int = 1):
    """nexg_encap_plan's offsets (count + 1 entries) for the output lengths."""
    offs = np.zeros(len(lengths) + 1, np.int64)
    for i, n in enumerate(lengths):
        offs[i + 1] = offs[i] + (int(n) + align - 1) // align * align
    return offs
