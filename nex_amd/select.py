"""Host side of frame selection and gather (include/nexg.h nexg_select_batch,
nexg_gather_plan / nexg_gather_frames / nexg_gather_rows).

An extension: the reference has no filter (examples/dump.rs prints every
frame), so there is no oracle for it. The contract in include/nexg.h is the
specification; match_host and gather_host restate it in plain Python, one
frame at a time, and are what the device output is tested against
(tests/golden/select_cases.json pins match_host itself by hand-derived cases).

Rule and Filter build the C structs and validate exactly as the C entry does
(ValueError where nexg_select_batch returns NEXG_EINVAL). There is no
expression-string parser.

    f = Filter([Rule.tcp(syn=True) & Rule.net("10.0.0.0/8", "dst"),   # TCP SYNs to 10/8
                Rule.udp() & Rule.port(53), Rule.udp() & Rule.port(5353),
                Rule.bad_checksum("l4"),
                Rule.net("2001:db8::/32", "src")])
"""
import ctypes
import ipaddress
from dataclasses import dataclass, field, fields
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import abi

TCP_FIN, TCP_SYN, TCP_RST, TCP_PSH, TCP_ACK, TCP_URG = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20

_ADDR_TESTS = abi.RULE_SRC_ADDR | abi.RULE_DST_ADDR | abi.RULE_ANY_ADDR
_PORT_TESTS = abi.RULE_SRC_PORT | abi.RULE_DST_PORT | abi.RULE_ANY_PORT
_DIRECTIONS = ("src", "dst", "any")


def _addr16(b) -> bytes:
    b = bytes(b)
    if len(b) > 16:
        raise ValueError("address longer than 16 bytes")
    return b + bytes(16 - len(b))


@dataclass
class Rule:
    """struct nexg_rule: a conjunction of tests (include/nexg.h)."""
    flags_mask: int = 0
    flags_value: int = 0
    tests: int = 0
    ip_proto: int = 0
    tcp_mask: int = 0
    tcp_value: int = 0
    family: int = 0
    src_bits: int = 0
    dst_bits: int = 0
    reserved: int = 0
    sport_lo: int = 0
    sport_hi: int = 0
    dport_lo: int = 0
    dport_hi: int = 0
    len_lo: int = 0
    len_hi: int = 0
    src: bytes = bytes(16)
    dst: bytes = bytes(16)

    # ---- the checks of nexg_select_batch -------------------------------------
    def validate(self) -> "Rule":
        t = self.tests
        for name, top in (("flags_mask", 32), ("flags_value", 32), ("tests", 32), ("ip_proto", 8), ("tcp_mask", 8),
                          ("tcp_value", 8), ("family", 8), ("src_bits", 8), ("dst_bits", 8), ("reserved", 16),
                          ("sport_lo", 16), ("sport_hi", 16), ("dport_lo", 16), ("dport_hi", 16), ("len_lo", 16),
                          ("len_hi", 16)):
            v = getattr(self, name)
            if not 0 <= int(v) < (1 << top):
                raise ValueError(f"rule: {name} = {v} does not fit its {top}-bit field")
        if len(bytes(self.src)) != 16 or len(bytes(self.dst)) != 16:
            raise ValueError("rule: src and dst are 16 bytes")
        if t & ~abi.RULE_ALL:
            raise ValueError("rule: unknown test bits")
        if self.reserved != 0:
            raise ValueError("rule: reserved must be 0")
        if t & abi.RULE_ANY_PORT and t & (abi.RULE_SRC_PORT | abi.RULE_DST_PORT):
            raise ValueError("rule: ANY_PORT excludes SRC_PORT and DST_PORT")
        if t & abi.RULE_ANY_PORT and (self.dport_lo or self.dport_hi):
            raise ValueError("rule: ANY_PORT needs dport_lo = dport_hi = 0")
        if t & (abi.RULE_SRC_PORT | abi.RULE_ANY_PORT) and self.sport_lo > self.sport_hi:
            raise ValueError("rule: sport_lo > sport_hi")
        if t & abi.RULE_DST_PORT and self.dport_lo > self.dport_hi:
            raise ValueError("rule: dport_lo > dport_hi")
        if t & abi.RULE_LENGTH and self.len_lo > self.len_hi:
            raise ValueError("rule: len_lo > len_hi")
        if t & abi.RULE_ANY_ADDR and t & (abi.RULE_SRC_ADDR | abi.RULE_DST_ADDR):
            raise ValueError("rule: ANY_ADDR excludes SRC_ADDR and DST_ADDR")
        if t & abi.RULE_ANY_ADDR and self.dst_bits:
            raise ValueError("rule: ANY_ADDR needs dst_bits = 0")
        if t & _ADDR_TESTS:
            if self.family not in (4, 6):
                raise ValueError("rule: address test with a family other than 4 or 6")
            width = 32 if self.family == 4 else 128
            if t & (abi.RULE_SRC_ADDR | abi.RULE_ANY_ADDR) and self.src_bits > width:
                raise ValueError("rule: src_bits above the family's width")
            if t & abi.RULE_DST_ADDR and self.dst_bits > width:
                raise ValueError("rule: dst_bits above the family's width")
        return self

    def to_c(self, validate=True) -> abi.RuleC:
        if validate:
            self.validate()
        c = abi.RuleC()
        for f in fields(self):
            v = getattr(self, f.name)
            if f.name in ("src", "dst"):
                setattr(c, f.name, (ctypes.c_uint8 * 16)(*bytes(v)[:16].ljust(16, b"\0")))
            else:
                width = 8 * getattr(abi.RuleC, f.name).size
                setattr(c, f.name, int(v) & ((1 << width) - 1))
        return c

    def __and__(self, other: "Rule") -> "Rule":
        """The conjunction of two rules, when one nexg_rule can hold it: no
        test kind in both, no address tests of two families, and flag bits
        both rules test must agree."""
        both = self.flags_mask & other.flags_mask
        if (self.flags_value ^ other.flags_value) & both:
            raise ValueError("rules test the same flag bits for different values")
        if self.tests & other.tests:
            raise ValueError("both rules carry the same test kind")
        if (self.tests & _ADDR_TESTS) and (other.tests & _ADDR_TESTS) and self.family != other.family:
            raise ValueError("address tests of two families in one rule")
        out = Rule(flags_mask=self.flags_mask | other.flags_mask, flags_value=self.flags_value | other.flags_value,
                   tests=self.tests | other.tests)
        for name in ("ip_proto", "tcp_mask", "tcp_value", "family", "src_bits", "dst_bits", "sport_lo", "sport_hi",
                     "dport_lo", "dport_hi", "len_lo", "len_hi"):
            setattr(out, name, getattr(self, name) or getattr(other, name))
        out.src = self.src if any(self.src) or self.tests & (abi.RULE_SRC_ADDR | abi.RULE_ANY_ADDR) else other.src
        out.dst = self.dst if any(self.dst) or self.tests & abi.RULE_DST_ADDR else other.dst
        return out.validate()

    # ---- convenience constructors ------------------------------------------------
    @classmethod
    def flags(cls, mask: int, value: Optional[int] = None) -> "Rule":
        """(record.flags & mask) == value (value defaults to mask: all set)."""
        return cls(flags_mask=mask, flags_value=mask if value is None else value).validate()

    @classmethod
    def tcp(cls, syn: Optional[bool] = None, ack: Optional[bool] = None, fin: Optional[bool] = None,
            rst: Optional[bool] = None) -> "Rule":
        """TCP frames; each of syn / ack / fin / rst given as True or False
        adds that TCP flag bit to the NEXG_RULE_TCP_FLAGS test."""
        r = cls(flags_mask=abi.L_TCP, flags_value=abi.L_TCP)
        for want, bit in ((syn, TCP_SYN), (ack, TCP_ACK), (fin, TCP_FIN), (rst, TCP_RST)):
            if want is not None:
                r.tests |= abi.RULE_TCP_FLAGS
                r.tcp_mask |= bit
                r.tcp_value |= bit if want else 0
        return r.validate()

    @classmethod
    def udp(cls) -> "Rule":
        return cls(flags_mask=abi.L_UDP, flags_value=abi.L_UDP).validate()

    @classmethod
    def proto(cls, ip_proto: int) -> "Rule":
        """IPv4 protocol / IPv6 next header as the record reports it."""
        return cls(tests=abi.RULE_PROTO, ip_proto=ip_proto).validate()

    @classmethod
    def port(cls, lo: int, hi: Optional[int] = None, direction: str = "any") -> "Rule":
        """TCP or UDP port in [lo, hi] (hi defaults to lo), as source,
        destination or either."""
        hi = lo if hi is None else hi
        if direction not in _DIRECTIONS:
            raise ValueError(f"direction must be one of {_DIRECTIONS}")
        if direction == "dst":
            return cls(tests=abi.RULE_DST_PORT, dport_lo=lo, dport_hi=hi).validate()
        return cls(tests=abi.RULE_SRC_PORT if direction == "src" else abi.RULE_ANY_PORT, sport_lo=lo,
                   sport_hi=hi).validate()

    @classmethod
    def net(cls, prefix: str, direction: str = "any") -> "Rule":
        """Address in a prefix such as "10.0.0.0/8" or "2001:db8::/32"."""
        if direction not in _DIRECTIONS:
            raise ValueError(f"direction must be one of {_DIRECTIONS}")
        n = ipaddress.ip_network(prefix, strict=False)
        a, bits, fam = _addr16(n.network_address.packed), n.prefixlen, 4 if n.version == 4 else 6
        if direction == "dst":
            return cls(tests=abi.RULE_DST_ADDR, family=fam, dst=a, dst_bits=bits).validate()
        return cls(tests=abi.RULE_SRC_ADDR if direction == "src" else abi.RULE_ANY_ADDR, family=fam, src=a,
                   src_bits=bits).validate()

    @classmethod
    def host(cls, address: str, direction: str = "any") -> "Rule":
        """One address (a /32 or /128 prefix)."""
        a = ipaddress.ip_address(address)
        return cls.net(f"{a}/{a.max_prefixlen}", direction)

    @classmethod
    def bad_checksum(cls, layer: str = "l4") -> "Rule":
        """Frames whose IPv4 header ("ip") or L4 ("l4") checksum was evaluated
        and does not equal the stored field."""
        if layer == "ip":
            return cls.flags(abi.C_IP_CHECKED | abi.C_IP_OK, abi.C_IP_CHECKED)
        if layer == "l4":
            return cls.flags(abi.C_L4_CHECKED | abi.C_L4_OK, abi.C_L4_CHECKED)
        raise ValueError('layer must be "ip" or "l4"')

    @classmethod
    def status(cls, code: int) -> "Rule":
        """Frames with this status (abi.FRAME_OK, abi.ERR_*)."""
        if not 0 <= code <= 7:
            raise ValueError("status is 0..7")
        return cls.flags(7 << abi.STATUS_SHIFT, code << abi.STATUS_SHIFT)

    @classmethod
    def length(cls, lo: int, hi: Optional[int] = None) -> "Rule":
        return cls(tests=abi.RULE_LENGTH, len_lo=lo, len_hi=lo if hi is None else hi).validate()

    @classmethod
    def any(cls) -> "Rule":
        """Matches every frame."""
        return cls()


@dataclass
class Filter:
    """struct nexg_filter: 1..16 rules, a frame matches when some rule does;
    invert flips the verdict."""
    rules: List[Rule] = field(default_factory=list)
    invert: bool = False
    flags: Optional[int] = None  # raw nexg_filter.flags; None = from `invert`

    def raw_flags(self) -> int:
        return (abi.FILTER_INVERT if self.invert else 0) if self.flags is None else self.flags

    def validate(self) -> "Filter":
        if not 1 <= len(self.rules) <= abi.FILTER_MAX_RULES:
            raise ValueError("filter: n_rules must be 1..16")
        if self.raw_flags() & ~abi.FILTER_INVERT:
            raise ValueError("filter: unknown flag bits")
        for r in self.rules:
            r.validate()
        return self

    def to_c(self, validate=True) -> abi.FilterC:
        if validate:
            self.validate()
        c = abi.FilterC()
        c.n_rules = len(self.rules) & 0xFFFFFFFF
        c.flags = self.raw_flags() & 0xFFFFFFFF
        for i, r in enumerate(self.rules[: abi.FILTER_MAX_RULES]):
            c.rules[i] = r.to_c(validate)
        return c


def _prefix(addr: bytes, want: bytes, bits: int) -> bool:
    n = len(addr)
    a, w = int.from_bytes(addr, "big"), int.from_bytes(bytes(want)[:n], "big")
    return (a >> (8 * n - bits)) == (w >> (8 * n - bits)) if bits else True


def rule_matches(frame: Optional[bytes], rec, length: int, r: Rule) -> bool:
    """One rule on one frame. `rec` is the frame's nexg_record (a numpy
    record or a dict), `frame` its bytes (None when the extent is not inside
    the batch's data), `length` len(i) as the frame table gives it."""
    flags = int(rec["flags"])
    if (flags & r.flags_mask) != r.flags_value:
        return False
    t = r.tests
    ok = (flags >> abi.STATUS_SHIFT) & 7 == 0  # an error record's fields carry the error's payload
    l4 = ok and bool(flags & (abi.L_TCP | abi.L_UDP))
    sport, dport = int(rec["src_port"]), int(rec["dst_port"])
    if t & abi.RULE_PROTO and not (ok and flags & (abi.L_IPV4 | abi.L_IPV6) and int(rec["ip_proto"]) == r.ip_proto):
        return False
    if t & abi.RULE_SRC_PORT and not (l4 and r.sport_lo <= sport <= r.sport_hi):
        return False
    if t & abi.RULE_DST_PORT and not (l4 and r.dport_lo <= dport <= r.dport_hi):
        return False
    if t & abi.RULE_ANY_PORT and not (l4 and (r.sport_lo <= sport <= r.sport_hi or r.sport_lo <= dport <= r.sport_hi)):
        return False
    if t & _ADDR_TESTS:
        if r.family == 4:
            if not (ok and flags & abi.L_IPV4):
                return False
            s, d = int(rec["ip_src"]).to_bytes(4, "big"), int(rec["ip_dst"]).to_bytes(4, "big")
        else:
            l3 = int(rec["l3_off"])
            if not (ok and flags & abi.L_IPV6 and frame is not None and length <= 65535 and l3 + 40 <= length):
                return False
            s, d = bytes(frame[l3 + 8: l3 + 24]), bytes(frame[l3 + 24: l3 + 40])
        if t & abi.RULE_SRC_ADDR and not _prefix(s, r.src, r.src_bits):
            return False
        if t & abi.RULE_DST_ADDR and not _prefix(d, r.dst, r.dst_bits):
            return False
        if t & abi.RULE_ANY_ADDR and not (_prefix(s, r.src, r.src_bits) or _prefix(d, r.src, r.src_bits)):
            return False
    if t & abi.RULE_TCP_FLAGS and not (ok and flags & abi.L_TCP and int(rec["l4_type"]) & r.tcp_mask == r.tcp_value):
        return False
    if t & abi.RULE_LENGTH and not r.len_lo <= length <= r.len_hi:
        return False
    return True


def match_host(frame: Optional[bytes], record, length: int, flt: Filter) -> Tuple[bool, int]:
    """nexg_select_batch's verdict for one frame: (selected, rule) with rule
    the lowest matching rule index, abi.RULE_NONE when no rule matches or the
    filter is inverted."""
    flt.validate()
    hit = next((i for i, r in enumerate(flt.rules) if rule_matches(frame, record, length, r)), abi.RULE_NONE)
    if flt.raw_flags() & abi.FILTER_INVERT:
        return hit == abi.RULE_NONE, abi.RULE_NONE
    return hit != abi.RULE_NONE, hit


def select_host(frames: Sequence[Optional[bytes]], records, lengths: Sequence[int], flt: Filter):
    """match_host over a batch: (index array, rule array) of the selected frames in order."""
    idx, rule = [], []
    for i, fr in enumerate(frames):
        sel, r = match_host(fr, records[i], int(lengths[i]), flt)
        if sel:
            idx.append(i)
            rule.append(r)
    return np.array(idx, np.uint32), np.array(rule, np.uint8)


def gather_host(data, offsets, lengths, align: int = 1):
    """nexg_gather_plan + nexg_gather_frames on the host: `data` the batch's
    bytes, offsets / lengths the selected table. Returns (out_offsets u64
    [count + 1], out_len u32 [count], out uint8 [total]): copied(k) = len(k),
    or 0 when the extent leaves the data or the length exceeds 65535; each
    frame's slot is rounded up to `align` with zero bytes."""
    if align not in abi.GATHER_ALIGNS:
        raise ValueError("align must be 1, 4, 8 or 16")
    buf = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data
    n = len(offsets)
    out_off = np.zeros(n + 1, np.uint64)
    out_len = np.zeros(n, np.uint32)
    pos = 0
    for k in range(n):
        o, ln = int(offsets[k]), int(lengths[k])
        bad = ln > 65535 or o < 0 or o > len(buf) or ln > len(buf) - o
        out_len[k] = 0 if bad else ln
        out_off[k] = pos
        pos += (int(out_len[k]) + align - 1) // align * align
    out_off[n] = pos
    out = np.zeros(pos, np.uint8)
    for k in range(n):
        o, c, d = int(offsets[k]), int(out_len[k]), int(out_off[k])
        out[d: d + c] = buf[o: o + c]
    return out_off, out_len, out
