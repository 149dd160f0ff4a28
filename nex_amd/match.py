"""Host side of the fixed-string match on frame bytes (include/nexg.h
nexg_match_batch / nexg_match_select).

An extension: the reference has no payload search, so there is no oracle for
it. The contract in include/nexg.h is the specification; match_host,
match_rows_host and match_select_host restate it in plain Python, one frame
and one byte at a time (no `re`), and are what the device output is tested
against (tests/test_match_host.py pins match_host by a hand-written truth
table and by an independent reference).

Pattern and PatternSet build the C structs and validate exactly as the C entry
does (ValueError where nexg_patterns_check returns NEXG_EINVAL).

    tls = PatternSet([Pattern.prefix(b"\\x16\\x03"),                  # payload starts with a TLS record
                      Pattern(b"Host: ", nocase=True),                # "host: " anywhere, any case
                      Pattern(b"\\r\\n\\r\\n", offset=(16, 512))])        # starting at payload bytes 16..512
"""
import ctypes
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import abi

ANYWHERE = (0, 65535)


@dataclass
class Pattern:
    """struct nexg_pattern: 1..16 bytes, compared at region-relative start
    positions offset[0]..offset[1] (both ends included)."""
    data: bytes
    nocase: bool = False
    offset: Tuple[int, int] = ANYWHERE
    flags: Optional[int] = None      # raw nexg_pattern.flags; None = from `nocase`
    reserved: bytes = bytes(10)      # raw nexg_pattern.reserved
    tail: bytes = b""                # raw bytes behind the pattern's own (must be 0)

    @classmethod
    def prefix(cls, data: bytes, nocase: bool = False) -> "Pattern":
        """The region starts with `data`."""
        return cls(data, nocase, (0, 0))

    @property
    def off_lo(self) -> int:
        return int(self.offset[0])

    @property
    def off_hi(self) -> int:
        return int(self.offset[1])

    def raw_flags(self) -> int:
        return (abi.PAT_NOCASE if self.nocase else 0) if self.flags is None else self.flags

    @property
    def folds(self) -> bool:
        return bool(self.raw_flags() & abi.PAT_NOCASE)

    def validate(self) -> "Pattern":
        if not 1 <= len(bytes(self.data)) <= abi.MATCH_MAX_LEN:
            raise ValueError("pattern: len must be 1..16")
        if any(bytes(self.tail)):
            raise ValueError("pattern: nonzero bytes past len")
        if not 0 <= self.raw_flags() < 256 or self.raw_flags() & ~abi.PAT_NOCASE:
            raise ValueError("pattern: unknown flag bits")
        if any(bytes(self.reserved)):
            raise ValueError("pattern: reserved must be 0")
        if not (0 <= self.off_lo <= 65535 and 0 <= self.off_hi <= 65535):
            raise ValueError("pattern: offsets are 16-bit")
        if self.off_lo > self.off_hi:
            raise ValueError("pattern: off_lo > off_hi")
        return self

    def to_c(self, validate=True) -> abi.PatternC:
        if validate:
            self.validate()
        c = abi.PatternC()
        data = bytes(self.data)
        body = (data + bytes(self.tail))[:16].ljust(16, b"\0") if len(data) <= 16 else data[:16]
        c.bytes = (ctypes.c_uint8 * 16)(*body)
        c.len = len(data) & 0xFF
        c.flags = self.raw_flags() & 0xFF
        c.off_lo = self.off_lo & 0xFFFF
        c.off_hi = self.off_hi & 0xFFFF
        c.reserved = (ctypes.c_uint8 * 10)(*bytes(self.reserved)[:10].ljust(10, b"\0"))
        return c


@dataclass
class PatternSet:
    """struct nexg_patterns: 1..32 patterns; frame=True searches the whole
    frame (NEXG_MATCH_FRAME) instead of Frame.payload."""
    patterns: List[Pattern] = field(default_factory=list)
    frame: bool = False
    flags: Optional[int] = None  # raw nexg_patterns.flags; None = from `frame`

    def raw_flags(self) -> int:
        return (abi.MATCH_FRAME if self.frame else 0) if self.flags is None else self.flags

    @property
    def whole_frame(self) -> bool:
        return bool(self.raw_flags() & abi.MATCH_FRAME)

    def validate(self) -> "PatternSet":
        if not 1 <= len(self.patterns) <= abi.MATCH_MAX_PATTERNS:
            raise ValueError("patterns: n_patterns must be 1..32")
        if self.raw_flags() & ~abi.MATCH_FRAME:
            raise ValueError("patterns: unknown flag bits")
        for p in self.patterns:
            p.validate()
        return self

    def to_c(self, validate=True) -> abi.PatternsC:
        if validate:
            self.validate()
        c = abi.PatternsC()
        c.n_patterns = len(self.patterns) & 0xFFFFFFFF
        c.flags = self.raw_flags() & 0xFFFFFFFF
        for i, p in enumerate(self.patterns[: abi.MATCH_MAX_PATTERNS]):
            c.pat[i] = p.to_c(validate)
        return c


NO_MATCH = (0, 0, abi.PAT_NONE)


def match_host(frame: Optional[bytes], record, length: int, pset: PatternSet) -> Tuple[int, int, int]:
    """nexg_match_batch's row for one frame: (mask, first_off, first_pat).
    `frame` is the frame's bytes (None when the extent is not inside the
    batch's data), `record` its nexg_record (a numpy record or a dict; not
    looked at under frame=True, may be None), `length` len(i) as the frame
    table gives it."""
    pset.validate()

    def fold(b):
        return b | 0x20 if 0x41 <= b <= 0x5A else b

    if frame is None or length > 65535:
        return NO_MATCH
    if pset.whole_frame:
        start, n = 0, length
    else:
        flags, off, ln = int(record["flags"]), int(record["payload_off"]), int(record["payload_len"])
        if (flags >> abi.STATUS_SHIFT) & 7 != 0 or ln == 0 or not off + ln <= length:
            return NO_MATCH
        start, n = off, ln
    hits = []  # (frame-relative offset, pattern) of every occurrence
    for i, p in enumerate(pset.patterns):
        want = [fold(b) if p.folds else b for b in bytes(p.data)]
        L = len(want)
        for q in range(n):
            if not (q + L <= n and p.off_lo <= q and q <= p.off_hi):
                continue
            k = 0
            while k < L and (fold(frame[start + q + k]) if p.folds else frame[start + q + k]) == want[k]:
                k += 1
            if k == L:
                hits.append((start + q, i))
    if not hits:
        return NO_MATCH
    mask = 0
    for _, i in hits:
        mask |= 1 << i
    first_off = min(o for o, _ in hits)
    first_pat = min(i for o, i in hits if o == first_off)
    return mask, first_off, first_pat


def match_rows_host(frames: Sequence[Optional[bytes]], records, lengths: Sequence[int], pset: PatternSet) -> np.ndarray:
    """match_host over a batch: nexg_match rows (abi.MATCH_DTYPE). `records`
    may be None under frame=True."""
    out = np.zeros(len(frames), abi.MATCH_DTYPE)
    for i, fr in enumerate(frames):
        m, o, p = match_host(fr, None if records is None else records[i], int(lengths[i]), pset)
        out[i] = (m, o, p, 0)
    return out


def row_selected(mask: int, any: int = 0, all: int = 0, none: int = 0) -> bool:  # noqa: A002 - the entry's words
    """nexg_match_select's predicate on one row's mask."""
    return (any == 0 or mask & any != 0) and mask & all == all and mask & none == 0


def match_select_host(rows, any: int = 0, all: int = 0, none: int = 0) -> np.ndarray:  # noqa: A002
    """nexg_match_select on the host: the indices of the selected frames, in order."""
    return np.array([i for i, m in enumerate(rows["mask"]) if row_selected(int(m), any, all, none)], np.uint32)
