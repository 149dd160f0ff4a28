"""Tunnelled test traffic: known inner frames (helpers.crafted_frames) wrapped
in VXLAN and GRE outer headers, with the negative and edge cases of
nexg_decap_batch (include/nexg.h). Every case carries what the wrapping
implies (tunnel kind, status, inner class, the inner bytes), so the
expectation does not come from the code under test."""
import json
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

from nex_amd import abi
from tests import helpers
from tests.helpers import _eth, _ipv4, _ipv6, _tcp

VECTORS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tunnel_vectors.json")


def vectors():
    with open(VECTORS) as f:
        return json.load(f)


@dataclass
class Case:
    frame: bytes            # the outer frame
    kind: int               # abi.TUN_* a default nexg_decap_batch reports (outer parsed with NEXG_PARSE_VLAN)
    status: int             # abi.FRAME_OK / ERR_MALFORMED
    inner_class: int        # abi.INNER_* (accepted tunnels)
    inner: Optional[bytes]  # the wrapped bytes (accepted tunnels)
    vlan: bool = False      # the outer headers carry a VLAN tag: a tunnel only with NEXG_PARSE_VLAN
    what: str = ""


def udp_to(payload: bytes, dport: int, sport: int = 0xC001) -> bytes:
    ln = 8 + len(payload)
    return sport.to_bytes(2, "big") + dport.to_bytes(2, "big") + ln.to_bytes(2, "big") + b"\x00\x00" + payload


def vxlan_header(vni: int, flags: int = 0x08, reserved1: int = 0, reserved2: int = 0) -> bytes:
    return bytes([flags]) + reserved1.to_bytes(3, "big") + vni.to_bytes(3, "big") + bytes([reserved2])


def gre_header(proto: int, c=0, k=0, s=0, r=0, version=0, checksum=0xC5C5, offset=0x0FF0, key=0xA1B2C3D4,
               seq=0x01020304) -> bytes:
    flags = c << 15 | r << 14 | k << 13 | s << 12 | version
    h = flags.to_bytes(2, "big") + proto.to_bytes(2, "big")
    if c or r:
        h += checksum.to_bytes(2, "big") + offset.to_bytes(2, "big")
    if k:
        h += key.to_bytes(4, "big")
    if s:
        h += seq.to_bytes(4, "big")
    return h


def outer_udp(payload: bytes, dport: int, v6: bool) -> bytes:
    u = udp_to(payload, dport)
    return _eth(_ipv6(u, 17), 0x86DD) if v6 else _eth(_ipv4(u, 17))


def outer_ip(payload: bytes, proto: int, v6: bool) -> bytes:
    return _eth(_ipv6(payload, proto), 0x86DD) if v6 else _eth(_ipv4(payload, proto))


def inner_sets():
    """(Ethernet frames, IPv4 packets, IPv6 packets): crafted_frames and their
    IP packets from byte 14 on."""
    eth = helpers.crafted_frames()
    ip4 = [f[14:] for f in eth if len(f) > 14 and f[12:14] == b"\x08\x00"]
    ip6 = [f[14:] for f in eth if len(f) > 14 and f[12:14] == b"\x86\xdd"]
    return eth, ip4, ip6


def cases():
    """The case list, kinds interleaved so that a short prefix is already varied."""
    eth, ip4, ip6 = inner_sets()
    T, OK, BAD = abi, abi.FRAME_OK, abi.ERR_MALFORMED
    combos = [(c, k, s) for c in (0, 1) for k in (0, 1) for s in (0, 1)]
    vx, g_eth, g_ip4, g_ip6, neg, tagged = [], [], [], [], [], []
    for i, f in enumerate(eth):
        h = vxlan_header(0x100 + i, reserved1=(i * 0x010203) & 0xFFFFFF, reserved2=i & 0xFF)
        vx.append(Case(outer_udp(h + f, 4789, i % 2 == 1), T.TUN_VXLAN, OK, T.INNER_ETHERNET, f, what=f"vxlan {i}"))
    for lst, inner, proto, cls in ((g_eth, eth, 0x6558, T.INNER_ETHERNET), (g_ip4, ip4, 0x0800, T.INNER_IPV4),
                                   (g_ip6, ip6, 0x86DD, T.INNER_IPV6)):
        for i, f in enumerate(inner):
            c, k, s = combos[i % 8]
            h = gre_header(proto, c, k, s, key=0xA1B2C300 + i, seq=0x7000000 + i)
            lst.append(Case(outer_ip(h + f, 47, (i // 8) % 2 == 1), T.TUN_GRE, OK, cls, f,
                            what=f"gre {proto:#x} cks={c}{k}{s} {i}"))
    # every C/K/S combination over both outer families, whatever the inner lists' lengths
    for j, (c, k, s) in enumerate(combos):
        for v6 in (False, True):
            f = eth[16 + j]
            g_eth.append(Case(outer_ip(gre_header(0x6558, c, k, s) + f, 47, v6), T.TUN_GRE, OK, T.INNER_ETHERNET, f,
                              what=f"gre all combos {c}{k}{s} v6={v6}"))
    inner = eth[16]  # Eth/IPv4/TCP
    vh = vxlan_header(0xABCDEF)
    for n in (0, 7):  # VxlanPacket::try_from_buf: fewer than 8 bytes -> None
        neg.append(Case(outer_udp(vh[:n], 4789, False), T.TUN_VXLAN, BAD, 0, None, what=f"vxlan payload {n} B"))
    neg.append(Case(outer_udp(vh, 4789, True), T.TUN_VXLAN, OK, T.INNER_ETHERNET, b"", what="vxlan payload exactly 8 B"))
    neg.append(Case(outer_udp(vh + inner, 4788, False), T.TUN_NONE, OK, 0, None, what="udp to another port"))
    neg.append(Case(outer_udp(vh + inner, 4790, False), T.TUN_NONE, OK, 0, None, what="udp to 4790 (custom port)"))
    neg.append(Case(outer_udp(vxlan_header(5, flags=0) + inner, 4789, False), T.TUN_VXLAN, OK, T.INNER_ETHERNET, inner,
                    what="vxlan I flag clear"))
    for c, k, s in combos:  # truncated inside each optional field (and inside the base header)
        full = gre_header(0x0800, c, k, s)
        for cut in range(len(full)):
            neg.append(Case(outer_ip(full[:cut], 47, (c + cut) % 2 == 1), T.TUN_GRE, BAD, 0, None,
                            what=f"gre cks={c}{k}{s} cut at {cut}"))
    for c, k, s in ((0, 0, 0), (1, 0, 0), (0, 1, 1)):  # the routing bit: None after the other fields
        neg.append(Case(outer_ip(gre_header(0x0800, c, k, s, r=1) + ip4[0], 47, False), T.TUN_GRE, BAD, 0, None,
                        what=f"gre routing bit cks={c}{k}{s}"))
    neg.append(Case(outer_ip(gre_header(0x0800, r=1)[:6], 47, True), T.TUN_GRE, BAD, 0, None, what="gre routing, short"))
    neg.append(Case(outer_ip(gre_header(0x880B, k=1, s=1, version=1) + b"\x11\x22\x33", 47, False), T.TUN_GRE, OK,
                    T.INNER_OTHER, b"\x11\x22\x33", what="gre version 1 (not checked)"))
    neg.append(Case(outer_ip(gre_header(0x0800, version=1) + ip4[3], 47, True), T.TUN_GRE, OK, T.INNER_IPV4, ip4[3],
                    what="gre version 1 ipv4"))
    neg.append(Case(outer_ip(gre_header(0x1234, c=1) + bytes(range(9)), 47, False), T.TUN_GRE, OK, T.INNER_OTHER,
                    bytes(range(9)), what="gre protocol 0x1234"))
    neg.append(Case(outer_ip(gre_header(0x6558), 47, False), T.TUN_GRE, OK, T.INNER_ETHERNET, b"", what="gre empty inner"))
    neg.append(Case(_eth(_ipv4(_tcp(bytes(20)), 6)), T.TUN_NONE, OK, 0, None, what="plain tcp"))
    neg.append(Case(_eth(bytes(range(28)), 0x0806), T.TUN_NONE, OK, 0, None, what="arp"))
    full = outer_udp(vh + inner, 4789, False)
    for n in (0, 13, 20, 40):
        neg.append(Case(full[:n], T.TUN_NONE, OK, 0, None, what=f"outer vxlan frame cut at {n}"))
    neg.append(Case(outer_ip(gre_header(0x0800) + ip4[0], 47, False)[:30], T.TUN_NONE, OK, 0, None,
                    what="outer gre frame cut inside the IPv4 header"))
    for i, c in enumerate((vx[16], vx[43], g_eth[17], g_ip4[2], g_ip6[1], neg[1], neg[9])):
        tagged.append(Case(helpers.vlan(c.frame, [0x0064 + i]), c.kind, c.status, c.inner_class, c.inner, vlan=True,
                           what="vlan " + c.what))
    groups = [vx, g_eth, g_ip4, neg, g_ip6, tagged]
    out = []
    for i in range(max(len(g) for g in groups)):
        out += [g[i] for g in groups if i < len(g)]
    return out


def cycled(case_list, count):
    """`count` cases cycled from the list; the last one an accepted tunnel, so
    that a packed batch ends with a tunnel on the final byte of its data."""
    c = [case_list[i % len(case_list)] for i in range(count)]
    if c:
        c[-1] = next(x for x in case_list if x.kind == abi.TUN_VXLAN and x.inner)
    return c


def tunnels_array(fields_list):
    """abi.TUNNEL_DTYPE array from decap_host's dicts."""
    a = np.zeros(len(fields_list), abi.TUNNEL_DTYPE)
    for i, t in enumerate(fields_list):
        for n in abi.TUNNEL_DTYPE.names:
            a[i][n] = t[n]
    return a
