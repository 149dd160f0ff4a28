"""Host side of IPv4 fragmentation to an MTU (include/nexg.h
nexg_fragment_plan / nexg_fragment_frames): RFC 791 section 3.2 over a table
of Ethernet frames, each piece the bytes the reference's Ipv4PacketBuilder
gives for its fields (Ipv4Flags::{DontFragment, MoreFragments},
fragment_offset, ipv4::checksum).

FragOption builds the C struct and validates exactly as the C entry does
(ValueError where nexg_frag_option_check returns NEXG_EINVAL). fragment_host
restates the contract of include/nexg.h in plain Python, one frame at a time,
and is what the device output is tested against (tests/test_fragment_host.py
pins it by a known answer, an independent reassembly and the oracle's parse).

    pieces, src, rows = fragment_host(frames, 1500)
"""
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import abi


@dataclass(frozen=True)
class FragOption:
    """struct nexg_frag_option."""
    mtu: int
    flags: int = 0
    align: int = 1
    reserved: int = 0

    def validate(self) -> "FragOption":
        """ValueError for what nexg_frag_option_check rejects."""
        if not abi.FRAG_MTU_MIN <= self.mtu <= abi.FRAG_MTU_MAX:
            raise ValueError("fragment: mtu must be 68..65535")
        if not 0 <= self.flags <= 0xFFFFFFFF or self.flags & ~abi.FRAG_IGNORE_DF:
            raise ValueError("fragment: unknown flag bits")
        if self.align not in abi.GATHER_ALIGNS:
            raise ValueError("fragment: align must be 1, 4, 8 or 16")
        if self.reserved:
            raise ValueError("fragment: reserved must be 0")
        return self

    def to_c(self, check=True) -> abi.FragOptionC:
        if check:
            self.validate()
        return abi.FragOptionC(mtu=self.mtu & 0xFFFFFFFF, flags=self.flags & 0xFFFFFFFF, align=self.align & 0xFFFFFFFF,
                               reserved=self.reserved & 0xFFFFFFFF)


def _be16(b: bytes, i: int) -> int:
    return b[i] << 8 | b[i + 1]


def header_checksum(header: bytes) -> int:
    """ipv4::checksum (ipv4.rs:932-938): the complement of the end-around sum of
    the header's big-endian words, the checksum field taken as 0."""
    s = 0
    for i in range(0, len(header), 2):
        if i != 10:
            s += _be16(header, i)
    while s >> 16:
        s = (s >> 16) + (s & 0xFFFF)
    return ~s & 0xFFFF


def later_options(options: bytes) -> bytes:
    """The options of a piece behind the first (rule 6): an option whose
    copied bit is clear becomes NOPs; the length stays."""
    o = bytearray(options)
    i = 0
    while i < len(o):
        t = o[i]
        if t == 0:
            break
        if t == 1:
            i += 1
            continue
        if i + 1 >= len(o):
            break
        n = o[i + 1]
        if n < 2 or n > len(o) - i:
            break
        if not t & 0x80:
            o[i:i + n] = b"\x01" * n
        i += n
    return bytes(o)


def fragment_frame(frame: Optional[bytes], mtu: int, ignore_df: bool = False):
    """Rules 1-6 of include/nexg.h for one frame: (pieces, status, kind, hl, p).
    `frame` None, or longer than 65535 bytes: an extent the table does not hold."""
    if frame is None or len(frame) > 65535:
        return [], abi.ERR_BAD_EXTENT, abi.FRAG_NONE, 0, 0
    f = bytes(frame)
    n = len(f)
    passed = ([f], abi.FRAME_OK, abi.FRAG_PASS, 0, 0)
    too_big = ([], abi.FRAME_OK, abi.FRAG_TOO_BIG, 0, 0)
    et = _be16(f, 12) if n >= 14 else -1
    if et == 0x86DD and n >= 54 and f[14] >> 4 == 6 and 40 + _be16(f, 18) <= n - 14:
        return too_big if 40 + _be16(f, 18) > mtu else passed
    if et != 0x0800 or n < 34 or f[14] >> 4 != 4 or f[14] & 15 < 5:
        return passed
    hl = 4 * (f[14] & 15)
    if 14 + hl > n:
        return passed
    total = _be16(f, 16)
    if total < hl or 14 + total > n:
        return passed
    if total <= mtu:
        return passed
    word = _be16(f, 20)
    reserved, df, mf0, fo0 = word & 0x8000, word & 0x4000, word & 0x2000, word & 0x1FFF
    if df and not ignore_df:
        return too_big
    data = f[14 + hl:14 + total]
    p = (mtu - hl) & ~7
    count = (len(data) + p - 1) // p
    if fo0 + (count - 1) * p // 8 > 8191:
        return [], abi.ERR_INVALID_LENGTH, abi.FRAG_NONE, 0, 0
    pieces = []
    for k in range(count):
        d = data[k * p:(k + 1) * p]
        h = bytearray(f[14:14 + hl])
        if k:
            h[20:] = later_options(bytes(h[20:]))
        h[2:4] = (hl + len(d)).to_bytes(2, "big")
        more = 0x2000 if k < count - 1 else mf0
        h[6:8] = (reserved | (0 if ignore_df else df) | more | (fo0 + k * p // 8)).to_bytes(2, "big")
        h[10:12] = header_checksum(bytes(h)).to_bytes(2, "big")
        pieces.append(f[:14] + bytes(h) + d)
    return pieces, abi.FRAME_OK, abi.FRAG_SPLIT, hl, p


def fragment_host(frames: Sequence[Optional[bytes]], mtu: int, ignore_df: bool = False):
    """nexg_fragment_plan + nexg_fragment_frames in plain Python: (pieces,
    src_index, rows). pieces: every output frame in order; src_index[f]: the
    input frame of output frame f; rows: an abi.FRAGGED_DTYPE array, one per
    input frame. `frames`: bytes, or None for an extent outside the data."""
    FragOption(mtu, abi.FRAG_IGNORE_DF if ignore_df else 0).validate()
    out: List[bytes] = []
    src: List[int] = []
    rows = np.zeros(len(frames), abi.FRAGGED_DTYPE)
    for i, f in enumerate(frames):
        pieces, status, kind, hl, p = fragment_frame(f, mtu, ignore_df)
        rows[i] = (status, kind, hl, 0, len(pieces), p, len(out), 0)
        out.extend(pieces)
        src.extend([i] * len(pieces))
    return out, np.array(src, np.uint32), rows


def plan_host(lengths: Sequence[int], align: int = 1):
    """The offsets (count + 1 entries) of output frames of these lengths, each start rounded up to `align`."""
    offs = np.zeros(len(lengths) + 1, np.int64)
    for i, n in enumerate(lengths):
        offs[i + 1] = offs[i] + (int(n) + align - 1) // align * align
    return offs
