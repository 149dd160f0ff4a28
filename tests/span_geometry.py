"""Geometry sweep of the parse kernels (nex_amd/csrc/parse_kernels.hpp): the
packed-span kernel k_parse_span (sub-tile loop, apron, head-window gather,
prefix values, bucketed generic pass, deferred ranges) and the two-pass path
(k_tail_sums' 256-B pieces and quarter-wave split, k_parse_lane80's window).
This module holds the constants the sweep restates, the probes, the builders
that put a probe at a stated position of the offset table, the geometry
classes (predicates on the table and the bytes) and the comparer.
tests/test_span_geometry.py checks all of it on the CPU;
tests/test_gpu_span_geometry.py runs the batches on the GPU.

Positions: a 256-frame group whose first frame starts at offset lo has its
origin at A0 = lo & ~15 (the data pointer is 16-B aligned), r(x) = x - A0, and
edge k of sub-tile size SUB is r = k * SUB, k >= 1. Whatever the kernels'
geometry is, it is restated here, so the constants below (pinned against the
sources by test_span_geometry.py) and GEOMETRY_CLASSES must move with it."""
from collections import namedtuple

import numpy as np

from nex_amd import abi

SPAN_SUB = {"record": 16384, "other": 24576}  # k_parse_span<RECORD, 16384, 1> / NEXG_SPAN_SUB
WIN = 84          # head-window gather: 21 dwords
SLOT = 80         # NEXG_SPAN_SLOT
LANE_WIN = 80     # kLaneWin
APRON = 96        # kApron
K_DEFER = 64      # SpanFrame::kDefer
K_PIECE = 256     # kPiece
TILE = 256        # kTile
BUCKETS = 9       # kBuckets
GUARD = 64        # untouched bytes required on both sides of every output
FILL = 0xA5

HEAD_DELTAS = tuple(range(-104, 13))
END_EPS = tuple(range(-17, 18))
SHIFTS = (0, 1, 4, 13)
PARTIAL_COUNTS = (1, 63, 64, 65, 255)
RANGE_LENGTHS = (65, 66, 255, 256, 257, 1023, 1024, 1025, 4000)
WAVE_DEFERRED = (1, 3, 4, 5, 8, 64)
TAIL_LENGTHS = (1, 15, 16, 17, 255, 256, 257, 65455)
PIECE_TOTALS = (0, 1, 2, 3, 4, 5, 6, 7)

# cls: geometry class; sub: the SUB the case aims at; k: edge; d: delta / epsilon
# (None where the class has none); probe: probe name; index: frame index in
# the batch; what: the frame-relative byte whose position the case states
# ("head" = 0, "end" = the frame length, "ip_end", "hi" = the group's last byte)
Case = namedtuple("Case", "cls sub k d probe index what")


def case_name(c):
    if c.k is None:  # classes 4, 5 and 7: a group or a wave, no edge
        return f"class {c.cls} {c.probe} ({c.what}, frame {c.index})"
    return f"class {c.cls} SUB {c.sub} edge k={c.k} d={c.d} probe {c.probe} ({c.what}, frame {c.index})"


# ---------------------------------------------------------------- frames

MACS = bytes(range(1, 13))
SRC4, DST4 = bytes([10, 1, 2, 3]), bytes([10, 4, 5, 6])
SRC6, DST6 = bytes(range(16)), bytes(range(16, 32))


def _sum16(b):
    if len(b) & 1:
        b = b + b"\0"
    return int(np.frombuffer(b, ">u2").sum(dtype=np.uint64))


def inet_checksum(*parts):
    """RFC 1071 over the concatenation (every part but the last of even length)."""
    s = sum(_sum16(p) for p in parts)
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return ~s & 0xFFFF


def eth(p, et=0x0800):
    return MACS + et.to_bytes(2, "big") + p


def ipv4(l4, proto, opts=b""):
    assert len(opts) % 4 == 0
    tot = 20 + len(opts) + len(l4)
    h = bytearray([0x45 + len(opts) // 4, 0, tot >> 8, tot & 255, 0x12, 0x34, 0x40, 0, 64, proto, 0, 0]) + SRC4 + DST4 + opts
    h[10:12] = inet_checksum(bytes(h)).to_bytes(2, "big")
    return bytes(h) + l4


def ipv6(l4, nh, ext=b""):
    plen = len(ext) + len(l4)
    return bytes([0x60, 0, 0, 0]) + plen.to_bytes(2, "big") + bytes([nh, 64]) + SRC6 + DST6 + ext + l4


def _pseudo(fam, proto, n):
    return (SRC4 + DST4 if fam == 4 else SRC6 + DST6) + bytes([0, proto]) + n.to_bytes(2, "big")


def udp(payload, fam=4):
    n = 8 + len(payload)
    h = b"\x04\xd2\x00\x35" + n.to_bytes(2, "big")
    c = inet_checksum(_pseudo(fam, 17, n), h + b"\0\0" + payload) or 0xFFFF
    return h + c.to_bytes(2, "big") + payload


def tcp(payload, opts=b"", fam=4):
    assert len(opts) % 4 == 0
    n = 20 + len(opts) + len(payload)
    h = bytes([0x12, 0x34, 0, 0x50, 1, 2, 3, 4, 5, 6, 7, 8, (5 + len(opts) // 4) << 4, 0x18, 0x20, 0])
    rest = b"\0\0" + opts + payload
    c = inet_checksum(_pseudo(fam, 6, n), h + b"\0\0" + rest)
    return h + c.to_bytes(2, "big") + rest


_POOL = np.random.default_rng(20240611).integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()


def _rand(n, seed):
    """n pool bytes (deterministic in seed): filler payloads need no fresh generator."""
    at = (seed * 7919) % (len(_POOL) - 65536)
    return _POOL[at: at + n]


def udp4_frame(n, seed=0):
    """A checksum-valid UDP/IPv4 frame of exactly n >= 42 bytes, pool payload."""
    assert 42 <= n <= 65535, n
    return eth(ipv4(udp(_rand(n - 42, seed)), 17))


_SHORT = {}


def _short(n):
    """udp4_frame(n, n), built once: the fillers that only fill a group up."""
    if n not in _SHORT:
        _SHORT[n] = udp4_frame(n, n)
    return _SHORT[n]


def padded(ip_end, frame_end, seed=0, tag=False):
    """UDP/IPv4 whose IP packet ends at frame byte ip_end, then non-zero
    Ethernet padding to frame_end (with tag: behind one 802.1Q tag)."""
    l3 = 18 if tag else 14
    ip = ipv4(udp(_rand(ip_end - l3 - 28, seed)), 17)
    head = MACS + (b"\x81\x00\x00\x64" if tag else b"") + b"\x08\x00"
    pad = bytes(b | 1 for b in _rand(frame_end - ip_end, seed + 1))
    return head + ip + pad


def probes():
    """{name: bytes} of the class-1 probes, every probe with bytes past 80
    also as <name>_bad with one of them corrupted (both verdicts occur)."""
    from tests import helpers
    rng = np.random.default_rng(11)
    ts = bytes([1, 1, 8, 10]) + _rand(8, 3)
    hbh, dst = bytes([60, 0, 1, 4, 0, 0, 0, 0]), bytes([17, 0, 1, 4, 0, 0, 0, 0])
    p = {
        "udp4_200": udp4_frame(200, 1),
        "tcp6_ts_300": eth(ipv6(tcp(_rand(300 - 86, 2), ts, 6), 6), 0x86DD),
        "udp4_60": udp4_frame(60, 4),
        "udp4_81": udp4_frame(81, 5),
        "pad64": padded(50, 64, 6),
        "pad_ip83_180": padded(83, 180, 7),
        "pad_ip84_180": padded(84, 180, 8),
        "pad_ip85_180": padded(85, 180, 9),
        "pad_ip120_180": padded(120, 180, 10),
        "tcp4_ipopt_400": eth(ipv4(tcp(_rand(400 - 58, 11)), 6, bytes([0x94, 4, 0, 0]))),
        "udp6_ext2_150": eth(ipv6(udp(_rand(150 - 78, 12), 6), 0, hbh + dst), 0x86DD),
        "arp42": eth(bytes([0, 1, 8, 0, 6, 4, 0, 1]) + bytes(range(20)), 0x0806),
        "len0": b"",
        "len1": b"\x45",
        "len13": bytes(range(13)),
        "vlan_tagged_pad": padded(200, 230, 13, tag=True),
        "vlan_untagged_pad": padded(200, 230, 14),
        "crafted_tcp4_ts": helpers.crafted_frames()[19],
        "fastpath_edge": next(f for f in helpers.fastpath_edge_frames(rng) if len(f) > 100),
        "tcp_option": helpers.tcp_walk_frames(rng)[0],
        "ipv4_option": next(f for f in helpers.ipv4_option_frames(rng) if len(f) > 120),
        "vlan_frame": helpers.vlan_frames()[1],
    }
    for name, f in list(p.items()):
        if len(f) > 80:
            g = bytearray(f)
            g[80 if len(f) == 81 else 81] ^= 0x5A
            p[name + "_bad"] = bytes(g)
    return p


PROBES = None


def probe(name):
    global PROBES
    if PROBES is None:
        PROBES = probes()
    return PROBES[name]


def ip_end_of(frame):
    """Frame byte where an untagged IPv4 packet ends (its total length)."""
    assert frame[12:14] == b"\x08\x00"
    return 14 + int.from_bytes(frame[16:18], "big")


# ---------------------------------------------------------------- placing frames

MIN_FILL = 42


class Layout:
    """Frames laid out one after another, `gap` bytes in front of each (0:
    packed), the first at `shift`; place() puts a frame byte at a stated
    position of its group with one sized filler in front. No case is ever
    dropped: a position that cannot be reached raises."""

    def __init__(self, sub, shift=0, gap=0):
        self.sub, self.gap = sub, gap
        self.pos = shift           # end of the last frame
        self.frames, self.offs, self.cases = [], [], []
        self.glo = None
        self.seed = 0

    @property
    def n(self):
        return len(self.frames)

    def add(self, frame):
        off = self.pos + self.gap
        if self.n % TILE == 0:
            self.glo = off
        self.offs.append(off)
        self.frames.append(frame)
        self.pos = off + len(frame)
        return self.n - 1

    def fill(self, n):
        self.seed += 1
        return self.add(udp4_frame(n, self.seed))

    def room(self, need):
        """At least `need` frames left in the current group (else it is filled up)."""
        if self.n % TILE and TILE - self.n % TILE < need:
            self.pad_group(0)

    def pad_group(self, until):
        """Short fillers until the group holds `until` frames (0: until it is full)."""
        while self.n % TILE != until % TILE:
            self.add(_short(MIN_FILL + self.n % 7))

    def place(self, cls, d, name, frame=None, at=0, what="head", last=False):
        """Frame byte `at` of the probe at r = k * SUB + d for the smallest
        reachable k >= 1. last: the probe becomes its group's last frame."""
        frame = probe(name) if frame is None else frame
        if last:
            if self.n % TILE > TILE - 2:
                self.pad_group(0)
            self.pad_group(TILE - 2)
        else:
            self.room(3)
        cur = self.pos + self.gap
        a0 = (cur if self.n % TILE == 0 else self.glo) & ~15
        k = 1
        while a0 + k * self.sub + d - at - self.gap - cur < MIN_FILL:
            k += 1
        want = a0 + k * self.sub + d - at - self.gap - cur
        while want > 65535:  # a filler frame holds 65535 B at most
            self.room(3)
            assert not last
            self.fill(32768)
            want -= 32768 + self.gap
        assert want >= MIN_FILL, (cls, d, name)
        self.fill(want)
        i = self.add(frame)
        assert self.offs[i] + at - a0 == k * self.sub + d, (cls, d, name)
        self.cases.append(Case(cls, self.sub, k, d, name, i, what))
        return i

    def table(self):
        """(data uint8, offsets u64 [count + 1 when packed], lengths u32 or None)."""
        total = self.pos
        data = np.zeros(max(total, 16), np.uint8)
        if self.gap == 0:
            at = self.offs[0] if self.offs else 0
            blob = b"".join(self.frames)
            data[at: at + len(blob)] = np.frombuffer(blob, np.uint8)
            return data[:max(total, 1)], np.array(self.offs + [self.pos], np.uint64), None
        data[:] = 0xC3  # the gaps (capture record headers) are not zero
        for o, f in zip(self.offs, self.frames):
            data[o: o + len(f)] = np.frombuffer(f, np.uint8)
        return data[:total], np.array(self.offs, np.uint64), np.array([len(f) for f in self.frames], np.uint32)


# the head sweep's probes on the shifted and the gapped layouts: one per path
# of the kernel (fast path with both verdicts, IP end as the second prefix
# position either side of its bound, declined with the range to the tail end,
# a window that ends inside the gather, nothing to gather). A shift moves no
# probe relative to its group's origin, so the full list runs unshifted only.
CORE_PROBES = ("udp4_200", "udp4_200_bad", "tcp6_ts_300_bad", "udp4_60", "udp4_81", "pad_ip83_180", "pad_ip84_180_bad",
               "tcp4_ipopt_400", "vlan_untagged_pad", "len0")
END_PROBES = ("udp4_200", "tcp4_ipopt_400", "pad_ip120_180", "vlan_untagged_pad")
SPAN_END_LAST = ("udp4_200", "udp4_60", "len0")


def head_sweep(lay, names=None):
    for name in (names or sorted(probes())):
        for d in HEAD_DELTAS:
            lay.place(1, d, name)
    return lay


def end_sweep(lay):
    for name in END_PROBES:
        f = probe(name)
        for e in END_EPS:
            lay.place(2, e, name, at=len(f), what="end")
        if name.startswith("pad") or name.startswith("vlan"):
            for e in END_EPS:
                lay.place(2, e, name, at=ip_end_of(f), what="ip_end")
    # the IP-end-120 probe with its IP end moved: every IP end from the window
    # end on, so r(off + ip_end) takes every phase at a fixed frame position too
    for ipe in range(84, 84 + 35):
        lay.place(2, END_EPS[ipe - 84], f"pad_ip{ipe}_180", frame=padded(ipe, 180, ipe), at=ipe, what="ip_end")
    return lay


def span_ends(lay):
    """Groups whose last byte lies at every epsilon of an edge, followed by
    another group (the batch goes on)."""
    for name in SPAN_END_LAST:
        f = probe(name)
        for e in END_EPS:
            lay.place(3, e, name, at=len(f), what="hi", last=True)  # (len0: its offset is the last byte)
            assert lay.n % TILE == 0
    lay.fill(64)  # the next group
    return lay


def span_end_batches(sub):
    """[(layout, count)] of small batches that end at hi: the data holds no
    byte past the last frame, and the last group is partial (2, 63, 64, 65,
    255 or all 256 frames; a batch of one frame ends on every epsilon too)."""
    out = []
    counts = (2, 63, 64, 65, 255, 256)
    i = 0
    for name in SPAN_END_LAST:
        f = probe(name)
        for e in END_EPS:
            lay = Layout(sub)
            n = counts[i % len(counts)]
            i += 1
            while lay.n < n - 2:
                lay.fill(MIN_FILL + lay.n % 7)
            lay.place(3, e, name, at=len(f), what="hi", last=n == TILE)
            out.append(lay)
    for e in END_EPS:  # one frame: the group is the frame
        lay = Layout(sub)
        lay.add(udp4_frame(sub + e, e + 40))
        lay.cases.append(Case(3, sub, 1, e, "udp4_single", 0, "hi"))
        out.append(lay)
    for n in PARTIAL_COUNTS:  # partial last groups behind a full one that ends on an edge
        lay = Layout(sub)
        lay.place(3, 0, "udp4_200", at=200, what="hi", last=True)
        for j in range(n - 1):
            lay.fill(MIN_FILL + j % 7)
        lay.add(probe("udp4_60"))
        assert lay.n == TILE + n
        out.append(lay)
    return out


def class123(sub, shift=0, gap=0):
    """The whole batch of classes 1-3 aimed at `sub` in one layout."""
    lay = Layout(sub, shift, gap)
    head_sweep(lay, None if shift == 0 and gap == 0 else CORE_PROBES)
    end_sweep(lay)
    span_ends(lay)
    return lay


def stride200():
    """(count, 200) uint8: the 200-B probes at a fixed stride the tile kernels
    refuse; frames 81, 122, 163 and 245 of every group cross an edge of one of
    the sub-tile sizes."""
    rows = [np.frombuffer(probe("udp4_200" if i % 3 else "udp4_200_bad"), np.uint8) for i in range(3 * TILE + 5)]
    return np.stack(rows)


# ---------------------------------------------------------------- class 4: prefix wrap

def prefix_wrap(shift):
    """Eight 65535-B UDP frames of all-0xFF payload among short ones, the
    first frame at an even or odd address."""
    lay = Layout(0, shift)
    big = eth(ipv4(udp(b"\xff" * (65535 - 42)), 17))
    for i in range(40):
        lay.add(big) if i % 5 == 2 else lay.fill(60 + i)
    lay.cases.append(Case(4, 0, None, shift, "udp4_65535_ff", 2, "head"))
    return lay


def prefix_wraps(data, offs):
    """Frames of a packed one-group batch in whose [80, len) range the running
    LE-halfword sum from the group's origin passes a multiple of 2^32."""
    a0 = int(offs[0]) & ~15
    b = data[a0: int(offs[-1])].astype(np.uint64)
    b[1::2] <<= np.uint64(8)  # a0 is even: absolute parity = index parity
    q = np.concatenate([[0], np.cumsum(b)])
    out = []
    for i in range(len(offs) - 1):
        lo, hi = int(offs[i]) + 80 - a0, int(offs[i + 1]) - a0
        if hi > lo and int(q[lo]) >> 32 != int(q[hi]) >> 32:
            out.append(i)
    return out


# ---------------------------------------------------------------- class 5: generic section

def span_bucket(frame, flags=0):
    """span_bucket (parse_kernels.hpp) of a declined frame."""
    if flags & abi.PARSE_FROM_IP or len(frame) < 14:
        return 8
    f = frame + bytes(24)
    if f[12:14] == b"\x08\x00":
        return {6: 0, 17: 1, 1: 2}.get(f[23], 3)
    if f[12:14] == b"\x86\xdd":
        return {6: 4, 17: 5, 58: 6}.get(f[20], 7)
    return 8


def declined_pool():
    """One frame per bucket that the fast path hands to the generic core (the
    CPU test asserts it from the host harness)."""
    ro = bytes([0x94, 4, 0, 0])
    two = bytes([2, 4, 5, 0xb4, 3, 3, 7, 0])  # two TLVs: the general option walk
    short = bytearray(udp(_rand(40, 26), 6))
    short[4:6] = (20).to_bytes(2, "big")  # bytes beyond the UDP length
    icmp6 = eth(ipv6(bytes([128, 0, 0, 0]) + _rand(24, 27), 58), 0x86DD) + bytes(18)  # IP end at 82 of 100 B
    ext = bytes([44, 0, 1, 4, 0, 0, 0, 0]) + bytes([17, 0, 0, 0, 0, 0, 0, 1])
    return [eth(ipv4(tcp(_rand(90, 21)), 6, ro)), eth(ipv4(udp(_rand(90, 22)), 17, ro)),
            eth(ipv4(bytes([8, 0, 0, 0]) + _rand(60, 23), 1, ro)), eth(ipv4(_rand(50, 24), 50, ro)),
            eth(ipv6(tcp(_rand(70, 25), two, 6), 6), 0x86DD), eth(ipv6(bytes(short), 17), 0x86DD), icmp6,
            eth(ipv6(udp(_rand(40, 28), 6), 60, ext), 0x86DD), probe("arp42")]


def generic_groups():
    """[(name, frames of one 256-frame group, lanes meant to be declined)]:
    the declined sets of class 5 among canonical (fast-path) UDP frames."""
    pool = declined_pool()
    fast = lambda i: udp4_frame(100 + i % 64, i)
    out = []

    def group(name, lanes, pick):
        fr = [fast(i) for i in range(TILE)]
        for j, t in enumerate(lanes):
            fr[t] = pick(j)
        out.append((name, fr, list(lanes)))

    for lane in (0, 63, 64, 255):
        group(f"one declined at lane {lane}", [lane], lambda j: pool[0])
    group("4 declined", [3, 70, 130, 200], lambda j: pool[j % 4])
    group("5 declined", [3, 70, 130, 200, 254], lambda j: pool[j % 5])
    group("one whole wave", range(64, 128), lambda j: pool[j % BUCKETS])
    group("all 256 in one bucket", range(TILE), lambda j: pool[1])
    group("all 256 over the 9 buckets", range(TILE), lambda j: pool[(j * 5) % BUCKETS])
    return out


def deferred_groups():
    """[(name, frames, deferred lanes)] for NEXG_PARSE_VLAN: padded UDP frames
    whose L4 range [80, IP end) is a deferred range of every length of
    RANGE_LENGTHS, 1, 3, 4, 5, 8 and 64 of them in the one worker wave; the
    fillers in front step the range start through every phase mod 16."""
    out = []
    k = 0
    for n in WAVE_DEFERRED:
        fr, lanes = [], []
        for t in range(TILE):
            if t % 4 == 1 and len(lanes) < n:
                ln = RANGE_LENGTHS[k % len(RANGE_LENGTHS)]
                fr.append(padded(80 + ln, 80 + ln + 5 + k % 3, 100 + k, tag=bool(k & 1)))
                lanes.append(t)
                k += 1
            else:
                fr.append(udp4_frame(90 + (t * 7 + n) % 16 + (t % 3), t + n))
        out.append((f"{n} deferred ranges in one worker wave", fr, lanes))
    return out


def packed(frames, shift=0):
    lay = Layout(0, shift)
    for f in frames:
        lay.add(f)
    return lay


# ---------------------------------------------------------------- class 7: two-pass path

def two_pass_batch():
    """(data, offsets u64, lengths u32, notes): offsets + lengths without the
    monotone hint. Every 64-frame wave lies in a region of its own whose start
    is a multiple of 256 (so is the wave base, the data pointer being 256-B
    aligned); notes = [(wave, what)]. Frame starts and lengths are chosen for
    their tail range [off + 80, off + len) against the 256-B piece edges and the
    16-B chunk edges."""
    waves, notes = [], []  # wave: list of (region-relative offset, frame) ; None offset = next free

    def tail_frame(ts, te, seed):
        """a frame whose tail range is [ts, te) region-relative: (offset, bytes)"""
        return ts - 80, udp4_frame(80 + te - ts, seed)

    # range starts and ends at -1, 0, +1 of a piece edge and of a chunk edge
    w = [tail_frame(256, 300, 1)]  # anchors the wave base at the region start + 256
    slot = 2048
    for s in (-1, 0, 1):
        for e in (-1, 0, 1):
            for edge in (256, 16):
                base = slot * len(w) + 1024
                w.append(tail_frame(base + edge + s, base + edge + 512 + e, len(w)))
    notes.append((len(waves), "range edges"))
    waves.append(w)
    # tail lengths
    w = [tail_frame(256, 260, 2)]
    at = 2048
    for ln in TAIL_LENGTHS:
        for ph in (0, 5):
            w.append(tail_frame(at + ph, at + ph + ln, len(w) + ln))
            at += (ln + 80 + 1023) // 1024 * 1024 + 1024
    notes.append((len(waves), "tail lengths"))
    waves.append(w)
    # piece totals 0..7: that many one-piece tails, the rest of the wave at most 80 B
    for total in PIECE_TOTALS:
        w = []
        for j in range(64):
            if j % 9 == 4 and sum(1 for _, f in w if len(f) > 80) < total:
                w.append(tail_frame(512 * j + 256 + 10, 512 * j + 256 + 40, j))
            else:
                w.append((512 * j + 100, udp4_frame(60 + j % 21, j)))
        assert sum(1 for _, f in w if len(f) > 80) == total
        notes.append((len(waves), f"piece total {total}"))
        waves.append(w)
    # one long frame at lane 0 / lane 63
    for lane in (0, 63):
        w = [(70000 + 256 * j, udp4_frame(70 + j, j)) for j in range(64)]
        w[lane] = (100, udp4_frame(65535, 9))
        notes.append((len(waves), f"long frame at lane {lane}"))
        waves.append(w)
    # decreasing address order
    w = [(1024 * (63 - j) + 3 * j, udp4_frame(150 + 5 * j, j)) for j in range(64)]
    notes.append((len(waves), "decreasing addresses"))
    waves.append(w)
    # the same frame named by two table rows
    w = [(1024 * (j // 2) + 7, udp4_frame(300 + j // 2, j // 2)) for j in range(64)]
    notes.append((len(waves), "duplicate rows"))
    waves.append(w)
    offs, lens, chunks, at = [], [], [], 0
    for w in waves:
        size = (max(o + len(f) for o, f in w) + 511) // 256 * 256
        reg = np.full(size, 0x3C, np.uint8)
        for o, f in w:
            assert o >= 0
            reg[o: o + len(f)] = np.frombuffer(f, np.uint8)
            offs.append(at + o)
            lens.append(len(f))
        while len(offs) % 64:  # waves are 64 table rows
            offs.append(at)
            lens.append(0)
        chunks.append(reg)
        at += size
    return np.concatenate(chunks), np.array(offs, np.uint64), np.array(lens, np.uint32), notes


def two_pass_pieces(offs, lens):
    """Per 64-frame wave the number of 256-B pieces k_tail_sums walks (the wave
    base: the lowest tail start rounded down to 256; the data pointer is 256-B
    aligned)."""
    out = []
    for w0 in range(0, len(offs), 64):
        o, n = offs[w0: w0 + 64].astype(np.int64), lens[w0: w0 + 64].astype(np.int64)
        have = n > LANE_WIN
        if not have.any():
            out.append(0)
            continue
        a, b = o[have] + LANE_WIN, o[have] + n[have]
        out.append(int(((b - 1) // K_PIECE - a // K_PIECE + 1).sum()))
    return out


def window_end_batches():
    """16 batches: a 60-B frame at every start phase, the data ending with it
    (k_parse_lane80's sixth load must not be issued past the batch)."""
    out = []
    for ph in range(16):
        fr = [udp4_frame(100, ph), udp4_frame(60, ph + 1)]
        data = np.full(256 + ph + 60, 0x3C, np.uint8)
        data[16: 116] = np.frombuffer(fr[0], np.uint8)
        data[256 + ph:] = np.frombuffer(fr[1], np.uint8)
        out.append((data, np.array([16, 256 + ph], np.uint64), np.array([100, 60], np.uint32)))
    return out


# ---------------------------------------------------------------- geometry classes

def _r(offs, i):
    g0 = i // TILE * TILE
    return int(offs[i]) - (int(offs[g0]) & ~15)


def position(c, offs, lens, frames):
    """r of the byte the case states, read from the table."""
    at = {"head": 0, "end": int(lens[c.index]), "hi": int(lens[c.index])}.get(c.what)
    if at is None:
        at = ip_end_of(frames[c.index])
    return _r(offs, c.index) + at


def _cases(lay, cls, what=None, pred=None):
    return [c for c in lay.cases if c.cls == cls and (what is None or c.what == what) and (pred is None or pred(c))]


def _covers(cs, values, names):
    have = {(c.probe, c.d) for c in cs}
    return all((n, v) in have for n in names for v in values)


def _last_gather(lay, sub):
    """a span-end case whose 60-B last frame has its head in the final 84 B of
    the last sub-tile (the `last && dh < SUB` gather)"""
    offs = lay.offs
    for c in _cases(lay, 3, pred=lambda c: c.probe == "udp4_60"):
        hi = _r(offs, c.index) + 60
        span = (hi + 15) & ~15
        s_last = (span - 1) // sub * sub
        dh = (_r(offs, c.index) & ~3) - s_last
        if sub - WIN - 4 < dh < sub:
            return True
    return False


# name -> predicate(layout of classes 1-3 aimed at sub, sub)
GEOMETRY_CLASSES = {
    "1 head sweep": lambda lay, sub: _covers(_cases(lay, 1), HEAD_DELTAS,
                                             sorted(probes()) if lay.offs[0] == 0 else CORE_PROBES),
    "1 in-place / apron switch": lambda lay, sub: {c.d < 0 for c in _cases(lay, 1)} == {True, False},
    "1 tail start both sides": lambda lay, sub: {c.d + LANE_WIN < 0 for c in _cases(lay, 1)} == {True, False},
    "2 frame end sweep": lambda lay, sub: _covers(_cases(lay, 2, "end"), END_EPS, END_PROBES),
    "2 ip end sweep": lambda lay, sub: _covers(_cases(lay, 2, "ip_end"), END_EPS,
                                               [p for p in END_PROBES if p[:3] in ("pad", "vla")]),
    "2 ip end from the window end on": lambda lay, sub: {ip_end_of(lay.frames[c.index])
                                                         for c in _cases(lay, 2, "ip_end")} >= set(range(84, 119)),
    "3 span end sweep": lambda lay, sub: _covers(_cases(lay, 3), END_EPS, ("udp4_200", "udp4_60", "len0")),
    "3 span == k * SUB": lambda lay, sub: any(c.d == 0 for c in _cases(lay, 3)),
    "3 last sub-tile 16 B": lambda lay, sub: any(1 <= c.d <= 16 for c in _cases(lay, 3)),
    "3 last-sub-tile gather": _last_gather,
}


# ---------------------------------------------------------------- the comparer

KINDS = (abi.OUT_RECORD, abi.OUT_DESC, abi.OUT_SPARSE, abi.OUT_GROUPED, abi.OUT_FLAGS, abi.OUT_VERDICT)
KIND_NAMES = {abi.OUT_RECORD: "record", abi.OUT_DESC: "desc", abi.OUT_SPARSE: "sparse", abi.OUT_GROUPED: "grouped",
              abi.OUT_FLAGS: "flags", abi.OUT_VERDICT: "verdict"}
_ITEM = {abi.OUT_RECORD: 64, abi.OUT_DESC: 8, abi.OUT_FLAGS: 4, abi.OUT_VERDICT: 2}


def flags_to_verdict(flags):
    """The 2-B verdict code of a flags word (include/nexg.h NEXG_OUT_VERDICT)."""
    flags = flags.astype(np.uint32)
    st = (flags >> np.uint32(abi.STATUS_SHIFT)) & np.uint32(7)
    return np.where(st != 0, np.uint32(abi.VERDICT_ERR) | (st << np.uint32(3)), flags & np.uint32(0xFFFF)).astype(np.uint16)


def out_bytes(kind, count):
    if kind == abi.OUT_SPARSE:
        return abi.sparse_bytes(count)
    if kind == abi.OUT_GROUPED:
        return abi.grouped_offsets(count)[3]
    return count * _ITEM[kind]


def decode(kind, body, count, lengths, flags=0, ip_offset=0):
    """A structured array of the output's per-frame fields."""
    if kind == abi.OUT_SPARSE:
        return abi.sparse_to_desc(body, count, lengths, flags, ip_offset)
    if kind == abi.OUT_GROUPED:
        return abi.grouped_to_desc(body, count, lengths, flags, ip_offset)
    dt = {abi.OUT_RECORD: abi.RECORD_DTYPE, abi.OUT_DESC: abi.DESC_DTYPE, abi.OUT_FLAGS: abi.FLAGS_DTYPE,
          abi.OUT_VERDICT: abi.VERDICT_DTYPE}[kind]
    return body[: count * dt.itemsize].view(dt)


def compare(kind, buf, want, lengths, cases=(), what="", flags=0, ip_offset=0, expanded=None):
    """Check a whole output buffer ([GUARD | output | GUARD], FILL before the
    call) bit for bit against the oracle's records `want`: every field the
    output kind carries, and both guards. expanded: the device expansion of a
    sparse / grouped output (nexg_desc bytes), checked the same way. A failure
    names the case of the first differing frame (or the case in front of it)
    and the first differing field."""
    count = len(want)
    n = out_bytes(kind, count)
    assert buf.dtype == np.uint8 and buf.shape == (GUARD + max(n, 16) + GUARD,), (buf.shape, n)
    by_index = {c.index: c for c in cases}

    def name_of(i):
        if i in by_index:
            return case_name(by_index[i])
        before = [c for c in cases if c.index < i]
        return f"frame {i}" + (f" (behind {case_name(max(before, key=lambda c: c.index))})" if before else "")

    def fail(msg):
        raise AssertionError(f"{what} {KIND_NAMES[kind]}: {msg}")

    def fields(got, tag):
        for f in got.dtype.names:
            ref = flags_to_verdict(want["flags"]) if f == "verdict" else want[f]
            bad = np.nonzero(got[f] != ref)[0]
            if bad.size:
                i = int(bad[0])
                first = next(g for g in got.dtype.names
                             if got[g][i] != (flags_to_verdict(want["flags"][i: i + 1])[0] if g == "verdict" else want[g][i]))
                fail(f"{tag}{bad.size} frames differ in {f}; first: {name_of(i)}, first differing field {first}: "
                     f"got {int(got[first][i]):#x} want "
                     f"{int(flags_to_verdict(want['flags'][i: i + 1])[0] if first == 'verdict' else want[first][i]):#x}")

    for side, g in (("before", buf[:GUARD]), ("after", buf[GUARD + max(n, 16):])):
        if (g != FILL).any():
            fail(f"guard byte {int(np.nonzero(g != FILL)[0][0])} {side} the output written"
                 + (f" ({case_name(cases[0])} ...)" if cases else ""))
    fields(decode(kind, buf[GUARD: GUARD + max(n, 16)], count, lengths, flags, ip_offset), "")
    if expanded is not None:
        fields(expanded[: count * 8].view(abi.DESC_DTYPE), "device expansion: ")


def host_buffer(kind, want):
    """The buffer a correct OUT_RECORD / OUT_DESC / OUT_FLAGS / OUT_VERDICT parse
    leaves (the CPU test seeds its defects into it)."""
    count = len(want)
    dt = {abi.OUT_RECORD: abi.RECORD_DTYPE, abi.OUT_DESC: abi.DESC_DTYPE, abi.OUT_FLAGS: abi.FLAGS_DTYPE,
          abi.OUT_VERDICT: abi.VERDICT_DTYPE}[kind]
    body = np.zeros(count, dt)
    for f in dt.names:
        body[f] = flags_to_verdict(want["flags"]) if f == "verdict" else want[f]
    buf = np.full(GUARD + max(count * dt.itemsize, 16) + GUARD, FILL, np.uint8)
    buf[GUARD: GUARD + count * dt.itemsize] = body.view(np.uint8)
    return buf


# ---------------------------------------------------------------- running a batch on the GPU

def device_batch(data, offs, lens=None, hints=0, stride=0, count=None):
    import torch
    from nex_amd.engine import FrameBatch
    dev = torch.from_numpy(np.ascontiguousarray(data)).cuda()
    assert dev.data_ptr() % 256 == 0  # the positions above assume it (16 B: spans, 256 B: piece edges)
    if offs is None:
        return FrameBatch(data=dev, count=count, stride=stride)
    ot = torch.from_numpy(offs.astype(np.int64)).cuda()
    lt = None if lens is None else torch.from_numpy(lens.astype(np.int32)).cuda()
    n = len(offs) - 1 if lens is None else len(offs)
    return FrameBatch(data=dev, count=n, offsets=ot, lengths=lt, hints=hints)


def run(engine, batch, kind, option=None, mode=None):
    """(whole host buffer with guards, device expansion or None)."""
    import torch
    from nex_amd.frame import ParseMode, ParseOption
    option, mode = option or ParseOption(), mode or ParseMode.Lenient
    n = max(out_bytes(kind, batch.count), 16)
    buf = torch.full((GUARD + n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    out = buf[GUARD: GUARD + n]
    engine.parse(batch, option, mode, kind, out=out)
    exp = None
    if kind in (abi.OUT_SPARSE, abi.OUT_GROUPED):
        exp = engine.sparse_expand(batch, out, option, mode, grouped=kind == abi.OUT_GROUPED)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), None if exp is None else exp.cpu().numpy()


def check(engine, batch, want, lengths, cases, what, kinds=KINDS, option=None, mode=None):
    from nex_amd.frame import ParseMode, ParseOption
    option, mode = option or ParseOption(), mode or ParseMode.Lenient
    for kind in kinds:
        buf, exp = run(engine, batch, kind, option, mode)
        compare(kind, buf, want, lengths, cases, what, option.flags(mode), option.offset, exp)
