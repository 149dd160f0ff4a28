"""TEST INFRASTRUCTURE ONLY: the corpus of the fixed-string match
(nexg_match_batch): Ethernet / IPv4 / UDP frames whose payload starts at frame
offset 42, with a few TCP, IPv6, error and non-IP frames. Every case is a
pattern set with the frames it runs over; tests/test_match_host.py holds the
corpus to its conditions (from an independent reference), the GPU tests run
the device over it against nex_amd.match.match_rows_host.

  sweep L      the pattern "abcdefghijklmnop"[:L] planted at every position q of
               a payload of n bytes of "." (n in SWEEP_N), whole where it fits
               and cut by the payload's end where it does not; behind a cut
               plant comes a frame that begins with exactly the missing bytes,
               so in the packed layout the pattern is complete in memory and
               only a reader that leaves the frame sees it
  header trap  patterns that straddle payload_off or lie in the headers: no hit
               in the payload, a hit under MATCH_FRAME
  shapes       ties, order, self-overlap, 16-byte with 1-byte, position windows
  nocase       hOsT: against HOST: / host:, the neighbours of the letters, bytes >= 0x80
  empty        payload_len 0, error status, a record edited to point past its frame
  large        one 65535-byte frame
  fuzz k       seeded random frames and sets of k patterns
"""
from dataclasses import dataclass, field
from typing import Callable, List, Optional

import numpy as np

from nex_amd import abi
from nex_amd.match import Pattern, PatternSet
from tests.helpers import _eth, _ipv4, _ipv6, _tcp, _udp

PARSE_FLAGS = abi.PARSE_VLAN | abi.PARSE_STRICT  # what helpers.parse_records parses with
PAYLOAD_OFF = 42
SWEEP_N = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 100)
SWEEP_L = (1, 2, 3, 4, 5, 8, 15, 16)
ALPHA = b"abcdefghijklmnop"
FUZZ_SIZES = (1, 2, 7, 16, 31, 32)
FUZZ_FRAMES = 2000


@dataclass
class Case:
    name: str
    pset: PatternSet
    frames: List[bytes]
    every_layout: bool = True                 # False: the first layout only (the fuzz sets)
    edit: Optional[Callable] = None           # applied to a copy of the oracle's records
    notes: dict = field(default_factory=dict)  # what the generator planted, for the conditions

    def records(self, oracle):
        recs = oracle.parse_frames(self.frames, PARSE_FLAGS).copy()
        if self.edit is not None:
            self.edit(recs)
        return recs


def udp(payload: bytes) -> bytes:
    return _eth(_ipv4(_udp(payload), 17))


def tcp(payload: bytes) -> bytes:
    return _eth(_ipv4(_tcp(payload), 6))


def udp6(payload: bytes) -> bytes:
    return _eth(_ipv6(_udp(payload), 17), 0x86DD)


def plant(n: int, q: int, pat: bytes, fill: bytes = b".") -> bytes:
    """n filler bytes with `pat` written at q, cut at n."""
    body = bytearray(fill * n)
    piece = pat[: max(0, n - q)]
    body[q: q + len(piece)] = piece
    return bytes(body)


def follower(head: bytes) -> bytes:
    """A frame that begins with `head` (a non-IP frame: the bytes are its MAC addresses)."""
    return head + b"." * (60 - len(head))


def sweep_case(L: int, frame: bool = False) -> Case:
    pat = ALPHA[:L]
    frames, planted = [], []
    for n in SWEEP_N:
        for q in range(n):
            frames.append(udp(plant(n, q, pat)))
            planted.append((n, q, q + L <= n))
            if q + L > n:  # cut by the region's end: the next frame begins with the missing bytes
                frames.append(follower(pat[n - q:]))
                planted.append(None)
    return Case(f"sweep L={L}" + (" frame" if frame else ""), PatternSet([Pattern(pat)], frame=frame), frames,
                notes={"planted": planted, "L": L})


def header_trap_cases() -> List[Case]:
    base = udp(b"." * 40)
    straddle = base[PAYLOAD_OFF - 3: PAYLOAD_OFF] + b"xyz"  # the UDP header's last 3 bytes, then the payload's first 3
    fr = udp(b"xyz" + b"." * 37)
    assert fr[PAYLOAD_OFF - 3: PAYLOAD_OFF + 3] == straddle
    inside = fr[14 + 12: 14 + 20]  # the two IPv4 addresses
    pats = [Pattern(straddle), Pattern(inside), Pattern(fr[:6]), Pattern(b"xyz")]
    frames = [fr, base, udp(b""), udp(b"xy"), tcp(b"xyz" * 5), udp6(b"..xyz")]
    return [Case("header trap payload", PatternSet(pats), frames),
            Case("header trap frame", PatternSet(pats, frame=True), frames)]


def shape_cases() -> List[Case]:
    out = []
    # 32 patterns that all occur at one position: the tie goes to pattern 0
    same = [Pattern(b"tie!"[: 1 + i % 4]) for i in range(32)]
    out.append(Case("32 at one position", PatternSet(same), [udp(b"..tie!.."), udp(b"tie"), udp(b"...t"), udp(b"none")]))
    # the higher index occurs earlier
    out.append(Case("higher index earlier", PatternSet([Pattern(b"late"), Pattern(b"early")]),
                    [udp(b".early..late."), udp(b"late.early"), udp(b"late"), udp(b"early"), udp(b"lat.earl")]))
    # self-overlap
    out.append(Case("aaa in aaaaa", PatternSet([Pattern(b"aaa"), Pattern(b"aaa", offset=(2, 2)), Pattern(b"aaa", offset=(3, 9))]),
                    [udp(b"aaaaa"), udp(b"aa"), udp(b".aaaa"), udp(b"aabaa")]))
    # a 16-byte and a 1-byte pattern in one set
    long16 = b"0123456789ABCDEF"
    out.append(Case("16 and 1", PatternSet([Pattern(long16), Pattern(b"F")]),
                    [udp(long16), udp(b"." + long16), udp(long16[:15]), udp(b"..." + long16 + b"F"), udp(b"F"),
                     udp(long16[1:] + long16)]))
    # position windows around a planted q
    q = 21
    win = [Pattern(b"mark", offset=(0, 0)), Pattern(b"mark", offset=(q, q)), Pattern(b"mark", offset=(q + 1, 65535)),
           Pattern(b"mark", offset=(0, q - 1)), Pattern(b"mark")]
    out.append(Case("windows", PatternSet(win),
                    [udp(plant(40, q, b"mark")), udp(plant(40, 0, b"mark")), udp(plant(40, q + 1, b"mark")),
                     udp(plant(40, q - 1, b"mark")), udp(plant(40, 36, b"mark")), udp(plant(40, 37, b"mark")),
                     udp(b"mark" + plant(40, q, b"mark"))]))
    return out


def nocase_cases() -> List[Case]:
    pats = [Pattern(b"hOsT:", nocase=True), Pattern(b"hOsT:"), Pattern(b"@[`{", nocase=True), Pattern(b"\xc4\xe4Z", nocase=True),
            Pattern(b"A", nocase=True, offset=(0, 0)), Pattern(b"z", nocase=True, offset=(0, 0))]
    texts = [b"HOST: x", b"host: x", b"GET / HOST:", b"hOsT:", b"hOsT", b"Hpst:", b"@[`{", b"`{@[", b"`[`{", b"@{`{", b"@[@{",
             b"\xc4\xe4z", b"\xc4\xe4Z", b"\xe4\xe4z", b"\xc4\xc4z", b"a", b"A", b"\x01", b"!", b"\xc1", b"\xe1", b"Z", b"z",
             b"\x1a", b"\x3a", b"\xda", b"\xfa", b"@", b"`", b"[", b"{"]
    return [Case("nocase", PatternSet(pats), [udp(t) for t in texts])]


def empty_cases() -> List[Case]:
    body = b"needle in a haystack"
    frames = [udp(b""), udp(body), udp(body), udp(body), _eth(_ipv4(_udp(body), 17))[:30], tcp(b""),
              udp(body), udp(body), udp(body)]

    def edit(recs):
        # frame 2: the payload would end one byte past the frame; 3: far past; 6: ends exactly at the frame's end
        # (still a region); 7: payload_off itself past the frame; 8: an error status over a whole payload
        recs["payload_len"][2] += 1
        recs["payload_off"][3] = 65535
        recs["payload_off"][6] += 4
        recs["payload_len"][6] -= 4
        recs["payload_off"][7] = len(frames[7])
        recs["payload_len"][7] = 1
        recs["flags"][8] |= abi.ERR_MALFORMED << abi.STATUS_SHIFT

    pats = [Pattern(b"needle"), Pattern(b"stack"), Pattern(b"e")]
    return [Case("empty regions", PatternSet(pats), frames, edit=edit),
            Case("empty regions frame", PatternSet(pats, frame=True), frames, edit=edit)]


def large_cases() -> List[Case]:
    n = 65535 - PAYLOAD_OFF
    L = 7
    pat = b"BigHit!"
    body = bytearray(b"." * n)
    where = (0, 32768 - PAYLOAD_OFF, n - L)
    for q in where:
        body[q: q + L] = pat
    big = udp(bytes(body))
    assert len(big) == 65535
    cut = bytearray(b"." * n)
    cut[n - L + 1:] = pat[: L - 1]  # cut by the frame's end; the follower completes it in memory
    frames = [udp(b"BigHit!"), big, follower(b"!"), udp(bytes(cut)), follower(b"!"), udp(b"Big")]
    pats = [Pattern(pat), Pattern(pat, offset=(1, 65535)), Pattern(pat, offset=(n - L, n - L)), Pattern(b"!", offset=(n - 1, n - 1))]
    return [Case("large", PatternSet(pats), frames, notes={"where": where, "L": L}),
            Case("large frame", PatternSet([Pattern(big[:6]), Pattern(pat, offset=(65535 - L, 65535))], frame=True), frames)]


FUZZ_ALPHABET = b"aAbB\x00\xff"


def _fuzz_pattern(rng, earlier):
    if earlier and rng.random() < 0.35:  # a prefix or a case variant of an earlier pattern: ties at one position
        src = earlier[int(rng.integers(len(earlier)))].data
        data = src[: int(rng.integers(1, len(src) + 1))]
        if rng.random() < 0.5:
            data = data.swapcase()
    else:
        ln = int(rng.choice([1, 2, 2, 3, 3, 4, 5, 6, 8, 11, 15, 16]))
        data = bytes(FUZZ_ALPHABET[int(i)] for i in rng.integers(0, len(FUZZ_ALPHABET), ln))
    r = rng.random()
    if r < 0.45:
        off = (0, 65535)
    elif r < 0.55:
        off = (0, 0)
    else:
        lo = int(rng.integers(0, 150))
        off = (lo, lo + int(rng.choice([0, 1, 7, 40, 65535 - lo])))
    return Pattern(data, nocase=bool(rng.random() < 0.4), offset=off)


def fuzz_case(k: int, seed: int = 2024) -> Case:
    rng = np.random.default_rng(seed + k)
    pats = []
    for _ in range(k):
        pats.append(_fuzz_pattern(rng, pats))
    frames = []
    for i in range(FUZZ_FRAMES):
        n = int(rng.integers(0, 201))
        # sparse filler: long runs of one byte, so that short patterns miss as well as hit
        fill = FUZZ_ALPHABET[int(rng.integers(len(FUZZ_ALPHABET)))]
        body = bytearray([fill]) * n
        for j in range(n):
            if rng.random() < 0.08:
                body[j] = FUZZ_ALPHABET[int(rng.integers(len(FUZZ_ALPHABET)))]
        for _ in range(int(rng.integers(0, 4))):
            p = pats[int(rng.integers(k))]
            data = p.data.swapcase() if p.nocase and rng.random() < 0.5 else p.data
            if n and rng.random() < 0.7 and p.off_lo < n:  # inside the pattern's window when the region reaches it
                q = int(rng.integers(p.off_lo, min(p.off_hi, n - 1) + 1))
            else:
                q = int(rng.integers(0, n + 1))
            piece = data[: max(0, n - q)]  # possibly cut by the end
            body[q: q + len(piece)] = piece
        kind = i % 23
        payload = bytes(body)
        if kind == 5:
            frames.append(tcp(payload))
        elif kind == 11:
            frames.append(udp6(payload))
        elif kind == 17:
            frames.append(udp(payload)[: 14 + int(rng.integers(0, 28))])  # cut inside the headers: an error status
        elif kind == 19:
            frames.append(_eth(payload, 0x88B5))  # not IP
        else:
            frames.append(udp(payload))
    return Case(f"fuzz {k}", PatternSet(pats), frames, every_layout=False)


def invalid_sets():
    """Every way nexg_patterns_check refuses a set, by name."""
    ok = Pattern(b"ok")
    return {
        "no patterns": PatternSet([]),
        "33 patterns": PatternSet([ok] * 33),
        "set flag 2": PatternSet([ok], flags=2),
        "set flag high": PatternSet([ok], flags=0x80000001),
        "len 0": PatternSet([ok, Pattern(b"")]),
        "len 17": PatternSet([Pattern(b"x" * 17)]),
        "bytes past len": PatternSet([Pattern(b"ab", tail=b"\0\0\1")]),
        "last byte past len": PatternSet([Pattern(b"ab", tail=bytes(13) + b"\x80")]),
        "pattern flag 2": PatternSet([Pattern(b"ab", flags=2)]),
        "pattern flag 0x81": PatternSet([Pattern(b"ab", flags=0x81)]),
        "reserved first": PatternSet([Pattern(b"ab", reserved=b"\1" + bytes(9))]),
        "reserved last": PatternSet([ok, Pattern(b"ab", reserved=bytes(9) + b"\1")]),
        "off_lo > off_hi": PatternSet([Pattern(b"ab", offset=(5, 4))]),
    }


_cache = {}


def cases() -> List[Case]:
    """Every case of the corpus (built once)."""
    if "all" not in _cache:
        out = [sweep_case(L) for L in SWEEP_L]
        out += [sweep_case(L, frame=True) for L in (1, 5, 16)]
        out += header_trap_cases() + shape_cases() + nocase_cases() + empty_cases() + large_cases()
        out += [fuzz_case(k) for k in FUZZ_SIZES]
        _cache["all"] = out
    return _cache["all"]


def case(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


def expected(oracle, c: Case):
    """(records, rows) of a case: the oracle's records with the case's edit,
    and nex_amd.match.match_rows_host over them (computed once per case)."""
    from nex_amd.match import match_rows_host
    key = ("rows", c.name)
    if key not in _cache:
        recs = c.records(oracle)
        _cache[key] = (recs, match_rows_host(c.frames, recs, [len(f) for f in c.frames], c.pset))
    return _cache[key]
