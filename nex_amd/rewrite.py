"""Host side of the header rewrite (include/nexg.h nexg_rewrite_batch): the
reference's mutable setters under ChecksumMode::Automatic, as a match-action
table's action half.

Action and ActionSet build the C structs and validate exactly as the C entry
does (ValueError where nexg_actions_check returns NEXG_EINVAL). rewrite_host
restates the contract of include/nexg.h in plain Python, one frame at a time,
and is what the device output is tested against (tests/test_rewrite_host.py
pins it by a hand-written truth table and by an independent reference).

    nat = Action.nat4(src="192.0.2.1", dst="198.51.100.7") & Action.ports(src=40000) & Action.dec_ttl(1)
    hop = Action.mac(dst="02:00:00:00:00:01", src="02:00:00:00:00:02") & Action.dec_ttl(1)
    actions = ActionSet([nat, hop, Action()])        # rule 2: leave it
"""
import ctypes
import ipaddress
from dataclasses import dataclass, field, replace
from typing import List, Optional

import numpy as np

from . import abi
from .frame import ParseOption

_ADDR = abi.SET_IP_SRC | abi.SET_IP_DST
_PORTS = abi.SET_SRC_PORT | abi.SET_DST_PORT
_IP_FIELDS = _ADDR | abi.SET_TTL | abi.DEC_TTL | abi.SET_TOS


def _mac(v) -> bytes:
    if isinstance(v, str):
        v = bytes(int(x, 16) for x in v.split(":"))
    v = bytes(v)
    if len(v) != 6:
        raise ValueError("action: a MAC address has 6 bytes")
    return v


def _ip(v, family) -> bytes:
    if isinstance(v, str):
        v = ipaddress.ip_address(v).packed
    v = bytes(v)
    if len(v) != (4 if family == 4 else 16):
        raise ValueError(f"action: an IPv{family} address has {4 if family == 4 else 16} bytes")
    return v


@dataclass(frozen=True)
class Action:
    """struct nexg_action. `sets` names the fields written (abi.SET_* /
    abi.DEC_TTL); the helpers build one field group each and `&` joins them
    (as Rule's `&`: every part applies)."""
    sets: int = 0
    family: int = 0
    ttl: int = 0
    tos: int = 0
    tos_mask: int = 0
    src_port: int = 0
    dst_port: int = 0
    eth_dst: bytes = bytes(6)
    eth_src: bytes = bytes(6)
    src: bytes = bytes(16)        # network order; family 4 uses the first 4 bytes
    dst: bytes = bytes(16)
    reserved: bytes = bytes(8)    # raw nexg_action.reserved

    # ---- builders ------------------------------------------------------------
    @classmethod
    def mac(cls, dst=None, src=None) -> "Action":
        """MutableEthernetPacket::set_destination / set_source."""
        a = cls()
        if dst is not None:
            a = replace(a, sets=a.sets | abi.SET_ETH_DST, eth_dst=_mac(dst))
        if src is not None:
            a = replace(a, sets=a.sets | abi.SET_ETH_SRC, eth_src=_mac(src))
        return a

    @classmethod
    def _nat(cls, family, src, dst) -> "Action":
        a = cls()
        if src is not None:
            a = replace(a, sets=a.sets | abi.SET_IP_SRC, family=family, src=_ip(src, family).ljust(16, b"\0"))
        if dst is not None:
            a = replace(a, sets=a.sets | abi.SET_IP_DST, family=family, dst=_ip(dst, family).ljust(16, b"\0"))
        return a

    @classmethod
    def nat4(cls, src=None, dst=None) -> "Action":
        """MutableIpv4Packet::set_source / set_destination (IPv4 frames only)."""
        return cls._nat(4, src, dst)

    @classmethod
    def nat6(cls, src=None, dst=None) -> "Action":
        """MutableIpv6Packet::set_source / set_destination (IPv6 frames only)."""
        return cls._nat(6, src, dst)

    @classmethod
    def ports(cls, src=None, dst=None) -> "Action":
        """MutableTcpPacket / MutableUdpPacket::set_source / set_destination."""
        a = cls()
        if src is not None:
            a = replace(a, sets=a.sets | abi.SET_SRC_PORT, src_port=int(src))
        if dst is not None:
            a = replace(a, sets=a.sets | abi.SET_DST_PORT, dst_port=int(dst))
        return a

    @classmethod
    def set_ttl(cls, ttl) -> "Action":
        """set_ttl / set_hop_limit."""
        return cls(sets=abi.SET_TTL, ttl=int(ttl))

    @classmethod
    def dec_ttl(cls, by=1) -> "Action":
        """TTL / hop limit lowered by `by`, not below 0."""
        return cls(sets=abi.DEC_TTL, ttl=int(by))

    @classmethod
    def set_tos(cls, tos, mask=0xFF) -> "Action":
        """(old & ~mask) | tos on the IPv4 TOS byte / IPv6 traffic class:
        mask 0xFC is set_dscp (tos = dscp << 2), mask 0x03 set_ecn."""
        return cls(sets=abi.SET_TOS, tos=int(tos), tos_mask=int(mask))

    def __and__(self, o: "Action") -> "Action":
        if self.sets & o.sets:
            raise ValueError("action: both parts set the same field")
        if self.family and o.family and self.family != o.family:
            raise ValueError("action: parts of different address families")
        pick = lambda bit, name: getattr(o if o.sets & bit else self, name)  # noqa: E731
        return Action(sets=self.sets | o.sets, family=self.family or o.family,
                      ttl=pick(abi.SET_TTL | abi.DEC_TTL, "ttl"), tos=pick(abi.SET_TOS, "tos"),
                      tos_mask=pick(abi.SET_TOS, "tos_mask"), src_port=pick(abi.SET_SRC_PORT, "src_port"),
                      dst_port=pick(abi.SET_DST_PORT, "dst_port"), eth_dst=pick(abi.SET_ETH_DST, "eth_dst"),
                      eth_src=pick(abi.SET_ETH_SRC, "eth_src"), src=pick(abi.SET_IP_SRC, "src"),
                      dst=pick(abi.SET_IP_DST, "dst"),
                      reserved=bytes(a | b for a, b in zip(bytes(self.reserved).ljust(8, b"\0"),
                                                           bytes(o.reserved).ljust(8, b"\0"))))

    # ---- the C form ----------------------------------------------------------
    def validate(self) -> "Action":
        if not 0 <= self.sets <= 0xFFFFFFFF or self.sets & ~abi.SET_ALL:
            raise ValueError("action: unknown sets bits")
        if any(bytes(self.reserved)):
            raise ValueError("action: reserved must be 0")
        if self.sets & abi.SET_TTL and self.sets & abi.DEC_TTL:
            raise ValueError("action: SET_TTL together with DEC_TTL")
        for name in ("ttl", "tos", "tos_mask", "family"):
            if not 0 <= getattr(self, name) <= 255:
                raise ValueError(f"action: {name} is 8-bit")
        for name in ("src_port", "dst_port"):
            if not 0 <= getattr(self, name) <= 65535:
                raise ValueError(f"action: {name} is 16-bit")
        if self.sets & abi.DEC_TTL and self.ttl == 0:
            raise ValueError("action: DEC_TTL by 0")
        if self.sets & _ADDR and self.family not in (4, 6):
            raise ValueError("action: an address set needs family 4 or 6")
        if not self.sets & _ADDR and self.family != 0:
            raise ValueError("action: a family without an address set")
        if self.sets & abi.SET_TOS and (self.tos_mask == 0 or self.tos & ~self.tos_mask):
            raise ValueError("action: SET_TOS with an empty mask or bits outside it")
        return self

    def to_c(self, validate=True) -> abi.ActionC:
        if validate:
            self.validate()
        c = abi.ActionC()
        c.sets = self.sets & 0xFFFFFFFF
        c.family, c.ttl, c.tos, c.tos_mask = self.family & 255, self.ttl & 255, self.tos & 255, self.tos_mask & 255
        c.src_port, c.dst_port = self.src_port & 0xFFFF, self.dst_port & 0xFFFF
        c.eth_dst = (ctypes.c_uint8 * 6)(*bytes(self.eth_dst)[:6].ljust(6, b"\0"))
        c.eth_src = (ctypes.c_uint8 * 6)(*bytes(self.eth_src)[:6].ljust(6, b"\0"))
        c.src = (ctypes.c_uint8 * 16)(*bytes(self.src)[:16].ljust(16, b"\0"))
        c.dst = (ctypes.c_uint8 * 16)(*bytes(self.dst)[:16].ljust(16, b"\0"))
        c.reserved = (ctypes.c_uint8 * 8)(*bytes(self.reserved)[:8].ljust(8, b"\0"))
        return c


@dataclass
class ActionSet:
    """struct nexg_actions: 1..16 actions; incremental=True updates the stored
    checksums by RFC 1624 (NEXG_REWRITE_INCREMENTAL) instead of recomputing."""
    actions: List[Action] = field(default_factory=list)
    incremental: bool = False
    flags: Optional[int] = None  # raw nexg_actions.flags; None = from `incremental`

    def raw_flags(self) -> int:
        return (abi.REWRITE_INCREMENTAL if self.incremental else 0) if self.flags is None else self.flags

    @property
    def is_incremental(self) -> bool:
        return bool(self.raw_flags() & abi.REWRITE_INCREMENTAL)

    def validate(self) -> "ActionSet":
        if not 1 <= len(self.actions) <= abi.REWRITE_MAX_ACTIONS:
            raise ValueError("actions: n_actions must be 1..16")
        if not 0 <= self.raw_flags() <= 0xFFFFFFFF or self.raw_flags() & ~abi.REWRITE_INCREMENTAL:
            raise ValueError("actions: unknown flag bits")
        for a in self.actions:
            a.validate()
        return self

    def to_c(self, validate=True) -> abi.ActionsC:
        if validate:
            self.validate()
        c = abi.ActionsC()
        c.n_actions = len(self.actions) & 0xFFFFFFFF
        c.flags = self.raw_flags() & 0xFFFFFFFF
        for i, a in enumerate(self.actions[: abi.REWRITE_MAX_ACTIONS]):
            c.actions[i] = a.to_c(validate)
        return c


# ---- the contract in plain Python -------------------------------------------------

def _be16(f, i):
    return f[i] << 8 | f[i + 1]


def _put16(f, i, v):
    f[i] = v >> 8 & 255
    f[i + 1] = v & 255


def _fold(t):
    while t >> 16:
        t = (t & 0xFFFF) + (t >> 16)
    return t


def _words(b):
    b = bytes(b)
    if len(b) & 1:
        b += b"\0"
    return sum(_be16(b, i) for i in range(0, len(b), 2))


def frame_views(f, flags=0, ip_offset=0):
    """The mutable views of one frame as the fix-up builds them (include/nexg.h):
    dict(eth, family, L, hl, P, m, proto, l4)."""
    n_f = len(f)
    v = dict(eth=False, family=0, L=14, hl=0, P=0, m=0, proto=0, l4=False)
    fam = 0
    if flags & abi.PARSE_FROM_IP:
        v["L"] = ip_offset
        ver = f[ip_offset] >> 4 if ip_offset < n_f else 0
        fam = ver if ver in (4, 6) else 0
    elif n_f >= 14:
        v["eth"] = True
        fam = {0x0800: 4, 0x86DD: 6}.get(_be16(f, 12), 0)
    L = v["L"]
    n = n_f - L if fam and L < n_f else 0
    if fam == 4 and n >= 20:
        hl, total = (f[L] & 15) * 4, _be16(f, L + 2)
        if hl >= 20 and hl <= n and (total == 0 or total >= hl):
            eff = n if total == 0 else min(total, n)
            v.update(family=4, hl=hl, P=L + hl, m=eff - hl, proto=f[L + 9])
            v["l4"] = v["proto"] in (17, 6, 1)
    elif fam == 6 and n >= 40:
        v.update(family=6, hl=40, P=L + 40, m=n - 40, proto=f[L + 6])
        v["l4"] = v["proto"] in (17, 6, 58)
    return v


def l4_view(f, v):
    """(the L4 view exists, byte offset of its checksum word) for frame_views' v with l4 set."""
    P, m = v["P"], v["m"]
    if v["proto"] == 17:
        ul = _be16(f, P + 4) if m >= 8 else 0
        return m >= 8 and (ul == 0 or 8 <= ul <= m), 6
    if v["proto"] == 6:
        hl = (f[P + 12] >> 4) * 4 if m >= 20 else 0
        return m >= 20 and 20 <= hl <= m, 16
    return m >= 8, 2


def _ip_checksum(f, v):
    L = v["L"]
    return ~_fold(_words(f[L:L + 10]) + _words(f[L + 12:L + v["hl"]])) & 0xFFFF


def _l4_checksum(f, v, sk):
    L, P, m = v["L"], v["P"], v["m"]
    t = _words(f[P:P + sk]) + _words(f[P + sk + 2:P + m])
    if v["proto"] != 1:
        t += _words(f[L + 12:L + 20] if v["family"] == 4 else f[L + 8:L + 40]) + v["proto"] + m
    return ~_fold(t) & 0xFFFF


def rewrite_frame_host(frame, action: Action, a: int, incremental=False, flags=0, ip_offset=0):
    """One frame under one action: (new bytes, (applied, fixed, action, ip_csum, l4_csum))."""
    f = bytearray(frame)
    if len(f) > 65535:  # an invalid extent
        return bytes(f), (0, 0, a, 0, 0)
    sets = action.sets
    v = frame_views(f, flags, ip_offset)
    L, P, fam = v["L"], v["P"], v["family"]
    applied = 0
    dip = dl4 = 0

    def put(i, nv):  # one 16-bit word; returns ~m + m'
        d = (~_be16(f, i) & 0xFFFF) + nv
        _put16(f, i, nv)
        return d

    if v["eth"]:
        if sets & abi.SET_ETH_DST:
            f[0:6] = action.eth_dst
            applied |= abi.SET_ETH_DST
        if sets & abi.SET_ETH_SRC:
            f[6:12] = action.eth_src
            applied |= abi.SET_ETH_SRC
    view, sk = False, 0
    if v["l4"]:
        later = incremental and fam == 4 and (_be16(f, L + 6) & 0x1FFF) != 0
        if not later:
            view, sk = l4_view(f, v)
    pseudo = v["proto"] != 1
    if fam and fam == action.family:
        nb = 4 if fam == 4 else 16
        so = L + 12 if fam == 4 else L + 8
        for bit, base, val in ((abi.SET_IP_SRC, so, action.src), (abi.SET_IP_DST, so + nb, action.dst)):
            if sets & bit:
                for k in range(0, nb, 2):
                    dip += put(base + k, _be16(val, k))
                applied |= bit
        if pseudo:
            dl4 = dip
    if fam and sets & (abi.SET_TTL | abi.DEC_TTL):
        i = L + (8 if fam == 4 else 7)
        old = f[i]
        nv = action.ttl if sets & abi.SET_TTL else max(old - action.ttl, 0)
        if fam == 4:
            dip += (~(old << 8 | f[i + 1]) & 0xFFFF) + (nv << 8 | f[i + 1])
        f[i] = nv
        applied |= sets & (abi.SET_TTL | abi.DEC_TTL)
    if fam and sets & abi.SET_TOS:
        if fam == 4:
            old = f[L + 1]
            nv = (old & ~action.tos_mask & 255) | action.tos
            dip += (~(f[L] << 8 | old) & 0xFFFF) + (f[L] << 8 | nv)
            f[L + 1] = nv
        else:
            old = (f[L] & 15) << 4 | f[L + 1] >> 4
            nv = (old & ~action.tos_mask & 255) | action.tos
            f[L] = (f[L] & 0xF0) | nv >> 4
            f[L + 1] = (f[L + 1] & 0x0F) | (nv & 15) << 4
        applied |= abi.SET_TOS
    if view and v["proto"] in (17, 6):
        if sets & abi.SET_SRC_PORT:
            dl4 += put(P, action.src_port)
            applied |= abi.SET_SRC_PORT
        if sets & abi.SET_DST_PORT:
            dl4 += put(P + 2, action.dst_port)
            applied |= abi.SET_DST_PORT

    ip_dirty = fam == 4 and applied & _IP_FIELDS
    l4_dirty = view and (applied & _PORTS or (applied & _ADDR and pseudo))
    fixed = ip_csum = l4_csum = 0
    if ip_dirty:
        if incremental:  # RFC 1624 eqn. 3
            ip_csum = ~_fold((~_be16(f, L + 10) & 0xFFFF) + dip) & 0xFFFF
        else:
            ip_csum = _ip_checksum(f, v)
        _put16(f, L + 10, ip_csum)
        fixed |= abi.FIX_IP
    if l4_dirty:
        if not incremental:
            l4_csum = _l4_checksum(f, v, sk)
            _put16(f, P + sk, l4_csum)
            fixed |= abi.FIX_L4
        else:
            hc = _be16(f, P + sk)
            if not (v["proto"] == 17 and fam == 4 and hc == 0):  # UDP over IPv4 "none" stays none
                l4_csum = ~_fold((~hc & 0xFFFF) + dl4) & 0xFFFF
                _put16(f, P + sk, l4_csum)
                fixed |= abi.FIX_L4
    return bytes(f), (applied, fixed, a, ip_csum, l4_csum)


def rewrite_host(frames, actions: ActionSet, index=None, option: ParseOption = ParseOption()):
    """nexg_rewrite_batch on the host: (new_frames, rows) with rows a
    REWRITTEN_DTYPE array. `index`: one action number per frame, or None
    (action 0 for every frame)."""
    actions.validate()
    flags = option.flags()
    rows = np.zeros(len(frames), abi.REWRITTEN_DTYPE)
    out = []
    for i, fr in enumerate(frames):
        a = 0 if index is None else int(index[i])
        if a >= len(actions.actions):
            out.append(bytes(fr))
            rows[i] = (0, 0, abi.ACTION_NONE, 0, 0)
            continue
        nf, row = rewrite_frame_host(fr, actions.actions[a], a, actions.is_incremental, flags, option.offset)
        out.append(nf)
        rows[i] = row
    return out, rows
