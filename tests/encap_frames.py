"""Encapsulation test traffic: the tunnel specs (every kind, both outer
families, every flag combination), the inner frames, and an independent
reference for nexg_encap_frames (include/nexg.h). The VXLAN outer frame is the
oracle's Eth / IPv4 / UDP or Eth / IPv6 / UDP builder around `VXLAN header +
inner`, the GRE outer frame is assembled here with the oracle's checksum for
the IPv4 header; nothing comes from nex_amd.encap.encap_host."""
import functools

import numpy as np

from nex_amd import abi
from nex_amd.encap import Tunnel, TunnelSet
from tests import helpers

M_DST, M_SRC = bytes.fromhex("02a0b0c0d0e1"), bytes.fromhex("02a0b0c0d0e2")
S4, D4 = "192.0.2.1", "198.51.100.7"
S6, D6 = "2001:db8::1", "2001:db8:0:ff::ffff:0:7"
EDGE_LENGTHS = (0, 1, 13, 14, 15, 16, 17, 31, 32, 33, 1500)


@functools.lru_cache(maxsize=None)
def specs():
    """24 specs: VXLAN x {4, 6} x {UDP_CSUM} x {FLOW_PORT}, GRE x {4, 6} x {K} x {S} x {L3}."""
    out = []
    for v6 in (False, True):
        for csum in (False, True):
            for flow in (False, True):
                k = len(out)
                out.append(Tunnel.vxlan(vni=(0xABCDEF, 5001, 0, 0xFFFFFF)[k % 4], src=S6 if v6 else S4, dst=D6 if v6 else D4,
                                        eth_dst=M_DST, eth_src=M_SRC, src_port=49152 + k, dst_port=0 if k % 2 else 8472,
                                        port_span=(16384 - k) if flow else 0, udp_csum=csum, ttl=64 - k, tos=(0, 0xB8)[k % 2],
                                        ip_id=0x1234 + k, ip_flags=(2, 0)[k % 2], flow_label=0xABCDE if k % 2 else 0))
    for v6 in (False, True):
        for K in (False, True):
            for S in (False, True):
                for l3 in (False, True):
                    k = len(out)
                    out.append(Tunnel.gre(src=S6 if v6 else S4, dst=D6 if v6 else D4, eth_dst=M_DST, eth_src=M_SRC,
                                          key=0xA1B2C300 + k if K else None,
                                          seq_base=(0xFFFFFFF0, 7)[k % 2] if S else None, l3=l3, ttl=255 - k,
                                          tos=(0x28, 0)[k % 2], ip_id=0xFFFF - k, ip_flags=(0, 2)[k % 2],
                                          flow_label=0xFFFFF if k % 2 else 0x12345))
    return tuple(out)


def spec_sets():
    """The specs as TunnelSets of at most 16, with each spec's number in specs()."""
    s = specs()
    return [(TunnelSet(s[:16]), list(range(16))), (TunnelSet(s[16:]), list(range(16, len(s))))]


def pattern(n, seed=0):
    """n bytes with no period of 2, 4 or 16 (a copy off by a phase shows)."""
    i = np.arange(n, dtype=np.uint32)
    return ((i * 131 + (i >> 8) * 17 + seed * 29 + 7) & 0xFF).astype(np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def small_inner():
    """crafted_frames and the edge lengths: Ethernet-shaped where 14 bytes fit."""
    eth = bytes(range(1, 13)) + b"\x08\x00"
    edge = [(eth + pattern(n, n))[:n] if n < 14 else eth + pattern(n - 14, n) for n in EDGE_LENGTHS]
    return tuple(helpers.crafted_frames() + edge)


def limit_inner(t: Tunnel):
    """The two inner frames at spec t's length limit: the longest that fits and one byte more."""
    n = 65535 - t.header_len() + (14 if t.l3_mode else 0)
    eth = bytes(range(1, 13)) + b"\x86\xdd"
    return [eth + pattern(n - 14, 1), eth + pattern(n + 1 - 14, 2)]


def be(v, n):
    return int(v).to_bytes(n, "big")


def ref_frame(oracle, inner: bytes, t: Tunnel, index: int = 0, flow_hash: int = 0, tunnel: int = 0):
    """(outer bytes, row tuple) for one in-extent frame under spec t, from the
    oracle's builders; the statuses follow the header's rules 2 and 3."""
    v4 = t.family == 4
    H = 14 + (20 if v4 else 40)
    if t.kind == abi.ENCAP_VXLAN:
        H += 16
        if H + len(inner) > 65535:
            return b"", (abi.ERR_INVALID_LENGTH, tunnel, 0, 0, 0, 0)
        port = t.src_port + (flow_hash % t.port_span if t.flags & abi.ENCAP_FLOW_PORT else 0)
        payload = b"\x08\x00\x00\x00" + be(t.id, 3) + b"\x00" + inner
        dport = t.dst_port or 4789
        if v4:
            out = oracle.build_udp4(t.eth_src, t.eth_dst, int.from_bytes(t.src[:4], "big"), int.from_bytes(t.dst[:4], "big"),
                                    port, dport, ip_id=t.ip_id, ttl=t.ttl, ip_flags=t.ip_flags, dscp_ecn=t.tos,
                                    payload=payload)
        else:
            out = oracle.build_udp6(t.eth_src, t.eth_dst, t.src, t.dst, port, dport, hop_limit=t.ttl, traffic_class=t.tos,
                                    flow_label=t.flow_label, payload=payload)
        at = H - 16 + 6
        csum = int.from_bytes(out[at:at + 2], "big")
        if not t.flags & abi.ENCAP_UDP_CSUM:
            out, csum = out[:at] + b"\x00\x00" + out[at + 2:], 0
        assert len(out) == H + len(inner)
        return out, (abi.FRAME_OK, tunnel, H, 0, port, csum)
    K, S, l3 = (bool(t.flags & b) for b in (abi.ENCAP_GRE_KEY, abi.ENCAP_GRE_SEQ, abi.ENCAP_GRE_L3))
    H += 4 + 4 * K + 4 * S
    if l3 and len(inner) < 14:
        return b"", (abi.ERR_BUFFER_TOO_SHORT, tunnel, 0, 0, 0, 0)
    payload = inner[14:] if l3 else inner
    if H + len(payload) > 65535:
        return b"", (abi.ERR_INVALID_LENGTH, tunnel, 0, 0, 0, 0)
    gre = be(K << 13 | S << 12, 2) + (inner[12:14] if l3 else b"\x65\x58")
    if K:
        gre += be(t.id, 4)
    if S:
        gre += be((t.seq_base + index) % (1 << 32), 4)
    l4 = gre + payload
    if v4:
        ip = bytearray(bytes([0x45, t.tos]) + be(20 + len(l4), 2) + be(t.ip_id, 2) + bytes([t.ip_flags << 5, 0, t.ttl, 47]) +
                       b"\x00\x00" + t.src[:4] + t.dst[:4])
        ip[10:12] = be(oracle.checksum(bytes(ip), 5), 2)
        et = b"\x08\x00"
    else:
        ip = (be(6 << 28 | t.tos << 20 | t.flow_label, 4) + be(len(l4), 2) + bytes([47, t.ttl]) + t.src + t.dst)
        et = b"\x86\xdd"
    return t.eth_dst + t.eth_src + et + bytes(ip) + l4, (abi.FRAME_OK, tunnel, H, 0, 0, 0)


def ref_all(oracle, frames, tunnels: TunnelSet, index=None, hashes=None):
    """The reference over a table: (outer frames, abi.ENCAPPED_DTYPE rows).
    None in `frames` is an extent outside the data; an index past the set a
    pass-through."""
    specs_ = list(tunnels.tunnels)
    out, rows = [], np.zeros(len(frames), abi.ENCAPPED_DTYPE)
    for i, f in enumerate(frames):
        n = 0 if index is None else int(index[i])
        if f is None:
            b, row = b"", (abi.ERR_BAD_EXTENT, n, 0, 0, 0, 0)
        elif n >= len(specs_):
            b, row = bytes(f), (abi.FRAME_OK, abi.TUNNEL_NONE, 0, 0, 0, 0)
        else:
            b, row = ref_frame(oracle, bytes(f), specs_[n], i, 0 if hashes is None else int(hashes[i]), n)
        out.append(b)
        rows[i] = row
    return out, rows


def hashes_for(n, seed=5):
    """Flow hash values with the FLOW_PORT edge values in front."""
    rng = np.random.default_rng(seed)
    h = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    edge = np.array([0, 1, 0xFFFFFFFF, 16383, 16384, 16385], np.uint32)
    h[: min(n, len(edge))] = edge[: min(n, len(edge))]
    return h


def flows_array(hashes):
    f = np.zeros(len(hashes), abi.FLOW_DTYPE)
    f["hash"] = hashes
    f["kind"] = abi.FLOW_IPV4_L4
    return f


def row_tuple(row):
    return tuple(int(row[n]) for n in abi.ENCAPPED_DTYPE.names)
