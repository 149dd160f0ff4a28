"""Differential sweep of the checksum fix-up (nexg_recompute_checksums_batch:
k_recompute, nex_amd/csrc/nexg_fixup.hip) and the checksum batch
(nexg_checksum_batch: k_checksum, nexg_parse.hip), which share
checksum_core.hpp's per-frame cores: the corpus (structured frames over the
payload lengths where global_le_sum's blocks, masks and accumulators change,
the 65535-B ceilings, planted fold edges, raw-IP variants behind odd
prefixes), two references (the oracle, and fixup_ref: a plain Python
restatement of include/nexg.h's view chain over re-assembled bytes), the host
layouts, the whole-buffer expectation and the comparer.
tests/test_fixup_sweep.py checks all of it on the CPU through the host harness;
tests/test_gpu_fixup_sweep.py runs it on the device."""
import functools
from collections import namedtuple

import numpy as np

from nex_amd import abi
from tests import helpers

BOTH = abi.FIX_IP | abi.FIX_L4
WHICH = (abi.FIX_IP, abi.FIX_L4, BOTH)
# payload lengths: around the 16-B block, the 4-B mask, 256 lanes' worth, the MTU and the 4 / 16 KiB marks
LENGTHS = (0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1471, 4095, 4096, 4097, 16383, 16384,
           16385, 40000)
RAW_OFFSETS = (0, 1, 13, 15, 21)       # raw_ip(k): ip_offset = k junk bytes ahead of the IP packet
MODES = [(False, 0), (True, 14)] + [(True, k) for k in RAW_OFFSETS]  # (from_ip, ip_offset); (True, 14): Ethernet corpus
GUARD_BEFORE, GUARD_AFTER, GUARD_FILL = 16, 64, 0xA5
MAX_FRAME = 65535

Planted = namedtuple("Planted", "frame layer target name")  # layer: "ip" / "l4"
Corpus = namedtuple("Corpus", "frames structured planted")  # structured: indices of the frames raw_ip() takes


def parse_flags(from_ip):
    return abi.PARSE_FROM_IP if from_ip else 0


# ---------------------------------------------------------------- frames

def _rnd(rng, n):
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


def _icmp(payload, typ=8, code=0):
    return bytes([typ, code, 0xBA, 0xD1, 0x12, 0x34, 0x00, 0x07]) + payload  # stored checksum: garbage


def _l4(kind, payload, doff=5):
    if kind == "udp":
        return helpers._udp(payload)
    if kind == "tcp":
        return helpers._tcp(payload, opts=bytes([1]) * (4 * doff - 20))
    return _icmp(payload)


PROTO = {"udp": 17, "tcp": 6, "icmp": 1}


def _v4(seg, proto, ihl=5, total=None, ident=0x1234):
    ip = bytearray(helpers._ipv4(seg, proto, ihl=ihl, opts=bytes([1]) * (4 * ihl - 20), total=total, ident=ident))
    ip[10:12] = b"\xba\xd2"  # stored header checksum: garbage
    return helpers._eth(bytes(ip))


def _v6(seg, nh):
    return helpers._eth(helpers._ipv6(seg, nh, plen=min(len(seg), 0xFFFF)), 0x86DD)


def structured_frames(rng):
    """The issue's grid over LENGTHS, then the 65535-B ceilings."""
    out = []
    for i, n in enumerate(LENGTHS):
        pay = _rnd(rng, n)
        for ihl in (5, 6, 15):
            for kind in ("udp", "tcp", "icmp"):
                out.append(_v4(_l4(kind, pay), PROTO[kind], ihl=ihl))
        out.append(_v6(_l4("udp", pay), 17))
        for doff in range(5, 16):
            out.append(_v6(_l4("tcp", pay, doff), 6))
        for typ in (128, 129, 135):  # echo request / reply, neighbour solicitation
            out.append(_v6(_icmp(pay, typ), 58))
        kind = ("udp", "tcp", "icmp")[i % 3]
        out.append(_v4(_l4(kind, pay), PROTO[kind], total=0))                          # total_length 0
        kind = ("tcp", "icmp", "udp")[i % 3]
        out.append(_v4(_l4(kind, pay), PROTO[kind]) + _rnd(rng, 1 + i % 9))            # trailing Ethernet padding
        seg = helpers._udp(pay, length=0)                                              # UDP length 0
        out.append(_v4(seg, 17) if i % 2 else _v6(seg, 17))
        out.append(_v4(pay, 50))                                                       # no L4 view: IP fix only
    room4, room6 = MAX_FRAME - 14 - 20, MAX_FRAME - 14 - 40
    out += [_v4(helpers._udp(_rnd(rng, room4 - 8)), 17),
            _v4(helpers._udp(_rnd(rng, room4 - 8)), 17, total=0),
            _v4(_icmp(_rnd(rng, room4 - 8)), 1),
            _v6(helpers._udp(_rnd(rng, room6 - 8)), 17),
            _v6(helpers._tcp(_rnd(rng, room6 - 20)), 6)]
    ones = bytearray(b"\xff" * MAX_FRAME)
    ones[12:15] = b"\x08\x00\x4f"  # IPv4, IHL 15: everything behind the IP header's first four bytes is 0xFF
    out.append(bytes(ones))        # protocol 255: the header sum alone
    ones[14 + 9] = 1               # and as ICMP: 65461 B of 0xFF in one L4 sum
    out.append(bytes(ones))
    assert all(len(f) == MAX_FRAME for f in out[-7:])
    return out


def _solve(oracle, frame, word_off, field_off, layer, target):
    """Set the 16-bit word at `word_off` (an even distance from the checksummed
    range's start) so that the oracle's recomputed checksum of `layer` is
    `target`; ones'-complement arithmetic from the oracle's own value."""
    f = bytearray(frame)
    _, rep = oracle.recompute_frame(bytes(f), BOTH)
    have = ~int(rep["ip_csum" if layer == "ip" else "l4_csum"]) & 0xFFFF
    want = ~target & 0xFFFF
    w = (int.from_bytes(f[word_off:word_off + 2], "big") + want - have) % 0xFFFF
    f[word_off:word_off + 2] = w.to_bytes(2, "big")
    fixed, rep = oracle.recompute_frame(bytes(f), BOTH)
    got = int(rep["ip_csum" if layer == "ip" else "l4_csum"])
    assert got == target and int.from_bytes(fixed[field_off:field_off + 2], "big") == target, (layer, target, got)
    assert bytes(f[field_off:field_off + 2]) != target.to_bytes(2, "big"), "the stored field must start as garbage"
    return bytes(f)


def planted_frames(oracle, rng):
    """Frames whose recomputed checksum is 0x0000 and 0x0001 for the IPv4
    header and every (family, protocol), and the all-zero ICMPv4 message
    (0xFFFF): the ends of fold_complement's range."""
    out = []
    for target in (0x0000, 0x0001):
        pay = _rnd(rng, 37)
        f = _v4(helpers._udp(pay), 17)
        out.append(Planted(_solve(oracle, f, 14 + 4, 14 + 10, "ip", target), "ip", target, f"ipv4 header {target:#06x}"))
        for fam in (4, 6):
            for kind in ("udp", "tcp", "icmp"):
                hdr = {"udp": 8, "tcp": 20, "icmp": 8}[kind]
                fld = {"udp": 6, "tcp": 16, "icmp": 2}[kind]
                body = _rnd(rng, 2 + int(rng.integers(0, 60)))
                if fam == 4:
                    f, l4 = _v4(_l4(kind, body), PROTO[kind]), 34
                else:
                    seg = _icmp(body, 128) if kind == "icmp" else _l4(kind, body)
                    f, l4 = _v6(seg, 58 if kind == "icmp" else PROTO[kind]), 54
                out.append(Planted(_solve(oracle, f, l4 + hdr, l4 + fld, "l4", target), "l4", target,
                                   f"ipv{fam} {kind} {target:#06x}"))
    zero = _v4(bytes([0, 0, 0xDE, 0xAD, 0, 0, 0, 0]), 1)
    _, rep = oracle.recompute_frame(zero, BOTH)
    assert int(rep["l4_csum"]) == 0xFFFF
    out.append(Planted(zero, "l4", 0xFFFF, "all-zero icmp 0xffff"))
    return out


@functools.lru_cache(maxsize=None)
def corpus():
    """The Ethernet corpus: structured and planted frames (the ones raw_ip()
    takes), the crafted / VLAN / FrameSlice edge cases and about 3000 mutations
    of the frames of at most 2 KiB."""
    from oracle import oracle
    rng = np.random.default_rng(1071)
    planted = planted_frames(oracle, rng)
    frames = structured_frames(rng) + [p.frame for p in planted]
    ns = len(frames)
    frames += helpers.crafted_frames() + helpers.vlan_frames() + helpers.slice_frames()
    small = [f for f in frames if len(f) <= 2048]
    frames += helpers.mutate_frames(rng, small, 3000)
    keep = [i for i, f in enumerate(frames) if len(f) <= MAX_FRAME]
    assert keep[:ns] == list(range(ns))
    return Corpus(tuple(frames[i] for i in keep), tuple(range(ns)), tuple(planted))


@functools.lru_cache(maxsize=None)
def raw_ip(k):
    """The structured frames' IP packets behind `k` junk bytes, for
    NEXG_PARSE_FROM_IP with ip_offset = k."""
    c = corpus()
    rng = np.random.default_rng(k)
    out = [_rnd(rng, k) + c.frames[i][14:] for i in c.structured]
    return tuple(f for f in out if len(f) <= MAX_FRAME)


def mode_frames(from_ip, ip_offset):
    """The corpus a (from_ip, ip_offset) mode runs over."""
    return corpus().frames if not from_ip or ip_offset == 14 else raw_ip(ip_offset)


# ---------------------------------------------------------------- references

_oracle_cache = {}


def oracle_fixed(frames, which, from_ip, ip_offset):
    """(fixed frames, nexg_fixup rows) from oracle.recompute_frame, computed
    once per corpus and mode and never modified."""
    from oracle import oracle
    key = (id(frames), which, from_ip, ip_offset)
    if key not in _oracle_cache:
        res = [oracle.recompute_frame(f, which, parse_flags(from_ip), ip_offset) for f in frames]
        rep = np.array([r for _, r in res], abi.FIXUP_DTYPE) if res else np.zeros(0, abi.FIXUP_DTYPE)
        rep.setflags(write=False)
        _oracle_cache[key] = (frames, tuple(b for b, _ in res), rep)
    return _oracle_cache[key][1:]


def rfc1071(data: bytes) -> int:
    """RFC 1071 over `data` as big-endian words (a trailing byte padded with zero)."""
    if len(data) % 2:
        data = data + b"\0"
    s = int(np.frombuffer(data, ">u2").sum(dtype=np.uint64))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return ~s & 0xFFFF


def fixup_ref(frame, which, from_ip=False, ip_offset=0):
    """include/nexg.h's mutable-view chain restated over re-assembled bytes:
    (fixed frame, (done, proto, ip_csum, l4_csum, l4_off))."""
    f = bytearray(frame)
    none = (bytes(f), (0, 0, 0, 0, 0))
    if from_ip:
        if ip_offset >= len(f):
            return none
        at, fam = ip_offset, f[ip_offset] >> 4
    else:
        if len(f) < 14:
            return none
        at, fam = 14, {0x0800: 4, 0x86DD: 6}.get(int.from_bytes(f[12:14], "big"), 0)
    n = len(f) - at
    done = ip_c = 0
    if fam == 4:
        if n < 20:
            return none
        hl, total = (f[at] & 15) * 4, int.from_bytes(f[at + 2:at + 4], "big")
        if hl < 20 or hl > n or (total and total < hl):
            return none
        if which & abi.FIX_IP:
            ip_c = rfc1071(bytes(f[at:at + 10]) + b"\0\0" + bytes(f[at + 12:at + hl]))
            f[at + 10:at + 12] = ip_c.to_bytes(2, "big")
            done |= abi.FIX_IP
        l4, m, proto = at + hl, (min(total, n) if total else n) - hl, f[at + 9]
        pseudo = bytes(f[at + 12:at + 20]) + bytes([0, proto]) + m.to_bytes(2, "big")
        known = (17, 6, 1)
    elif fam == 6:
        if n < 40:
            return none
        l4, m, proto = at + 40, n - 40, f[at + 6]
        pseudo = bytes(f[at + 8:at + 40]) + m.to_bytes(4, "big") + bytes([0, 0, 0, proto])
        known = (17, 6, 58)
    else:
        return none
    rep = (done, 0, ip_c, 0, 0)
    if not which & abi.FIX_L4 or proto not in known:
        return bytes(f), rep
    seg = bytes(f[l4:l4 + m])
    if proto == 17:
        ul = int.from_bytes(seg[4:6], "big") if m >= 8 else 0
        view, field = m >= 8 and (ul == 0 or 8 <= ul <= m), 6
    elif proto == 6:
        view, field = m >= 20 and 20 <= (seg[12] >> 4) * 4 <= m, 16
    else:
        view, field = m >= 8, 2
    if not view:
        return bytes(f), rep
    c = rfc1071((b"" if proto == 1 else pseudo) + seg[:field] + b"\0\0" + seg[field + 2:])
    f[l4 + field:l4 + field + 2] = c.to_bytes(2, "big")
    return bytes(f), (done | abi.FIX_L4, proto, ip_c, c, l4)


def report_row(rep):
    """A nexg_fixup row as fixup_ref's tuple."""
    return tuple(int(rep[n]) for n in ("done", "proto", "ip_csum", "l4_csum", "l4_off"))


# ---------------------------------------------------------------- corpus conditions

def check_corpus():
    """What the sweep relies on the corpus to hold (asserted by the CPU test
    and again before the GPU sweep)."""
    c = corpus()
    _, rep = oracle_fixed(c.frames, BOTH, False, 0)
    lens = np.array([len(f) for f in c.frames])
    for done, protos in ((0, (0,)), (abi.FIX_IP, (0,)), (abi.FIX_L4, (6, 17, 58)), (BOTH, (1, 6, 17))):
        for p in protos:
            n = int(((rep["done"] == done) & (rep["proto"] == p)).sum())
            assert n >= 100, f"class (done {done}, proto {p}) holds {n} frames"
    long_l4 = int((((rep["done"] & abi.FIX_L4) != 0) & (lens > 16384)).sum())
    assert long_l4 >= 20, long_l4
    index = {f: i for i, f in reversed(list(enumerate(c.frames)))}
    for p in c.planted:
        r = rep[index[p.frame]]
        got = int(r["ip_csum"] if p.layer == "ip" else r["l4_csum"])
        assert got == p.target and int(r["done"]) & (abi.FIX_IP if p.layer == "ip" else abi.FIX_L4), (p.name, got)
    for k in RAW_OFFSETS:
        fr = raw_ip(k)
        _, rr = oracle_fixed(fr, BOTH, True, k)
        v6 = np.array([len(f) > k and f[k] >> 4 == 6 for f in fr])
        assert int((rr["done"] == BOTH).sum()) >= 100, k
        assert int((((rr["done"] & abi.FIX_L4) != 0) & v6).sum()) >= 100, k
    assert sum(lens) < 32 << 20
    return rep


# ---------------------------------------------------------------- checksum batch cases

# want: None = the oracle's value, else the value the kernel's extent rule gives
Buffer = namedtuple("Buffer", "data skipword want")


@functools.lru_cache(maxsize=None)
def checksum_cases():
    rng = np.random.default_rng(65)
    out = []
    for n in LENGTHS + (MAX_FRAME,):
        for data in (_rnd(rng, n), b"\xff" * n, bytes(n)):
            skips = {0, 1, 3, 5, 8, max(n // 2 - 1, 0), n // 2, 2**32 - 1}
            if n % 2:
                skips.add((n - 1) // 2)  # the trailing partial word: its one byte is dropped
            out += [Buffer(data, s, None) for s in sorted(skips)]
    out += [Buffer(_rnd(rng, 65536), 1, 0), Buffer(b"", 0, 0)]  # out of range: 0 (k_checksum's extent rule, util.rs:66)
    return tuple(out)


def checksum_ref(data: bytes, skipword: int) -> int:
    """RFC 1071 with the skipped word zeroed; a skipped word that starts at the
    last byte of an odd-length buffer takes that byte with it; empty: 0."""
    if not data:
        return 0
    b = bytearray(data)
    if 2 * skipword < len(b):
        b[2 * skipword:2 * skipword + 2] = bytes(len(b[2 * skipword:2 * skipword + 2]))
    return rfc1071(bytes(b))


# ---------------------------------------------------------------- host layouts

Layout = namedtuple("Layout", "name data offsets lengths stride table keep")
# offsets / lengths: every kept frame's extent in `data` (int64); table: the harness.recompute / checksum keywords


def aligned(n, fill=0):
    """A uint8 array of n bytes at a 16-B aligned address (the kernels' load
    granule: the host harness reads whole aligned 16-B blocks)."""
    raw = np.full(n + 16, fill, np.uint8)
    o = -raw.ctypes.data % 16
    return raw[o:o + n]


def copy_aligned(a):
    out = aligned(len(a))
    out[:] = a
    return out


def pack(frames, shift=0, pad_to=1, tail=16):
    """(data, count + 1 offsets): the frames back to back from byte `shift`,
    each start a multiple of pad_to past it, `tail` spare bytes behind."""
    offs = np.zeros(len(frames) + 1, np.int64)
    offs[1:] = np.cumsum([(len(f) + pad_to - 1) // pad_to * pad_to for f in frames])
    offs += shift
    buf = aligned(int(offs[-1]) + tail)
    for f, o in zip(frames, offs):
        buf[o:o + len(f)] = np.frombuffer(f, np.uint8)
    return buf, offs


def host_layouts(frames, shift=1, strided_below=4096):
    """Every frame_extent class over host arrays: packed u64 / u32 (with and
    without group bases), offsets + lengths in u64 and u32, fixed stride with
    and without lengths. The first frame starts `shift` bytes into `data`."""
    lens = np.array([len(f) for f in frames], np.int64)
    out = []
    buf, offs = pack(frames, shift)
    for name, kw in (("packed u64", {}), ("packed u32", {"offsets32": True}),
                     ("packed u32 + bases", {"offsets32": True, "bases": True})):
        out.append(Layout(name, copy_aligned(buf), offs[:-1], lens, 0, dict(offsets=offs, **kw), None))
    buf, offs = pack(frames, shift, pad_to=4)
    for name, kw in (("offsets + lengths u64", {}), ("offsets32 + lengths", {"offsets32": True})):
        out.append(Layout(name, copy_aligned(buf), offs[:-1], lens, 0, dict(offsets=offs, lengths=lens, **kw), None))
    keep = np.array([i for i, f in enumerate(frames) if len(f) < strided_below], np.int64)
    if len(keep):
        stride = (int(lens[keep].max()) + 16) // 16 * 16
        a = aligned(len(keep) * stride).reshape(len(keep), stride)
        for r, i in enumerate(keep):
            a[r, :lens[i]] = np.frombuffer(frames[i], np.uint8)
        so = np.arange(len(keep), dtype=np.int64) * stride
        out.append(Layout("strided + lengths", a.reshape(-1), so, lens[keep], stride,
                          dict(stride=stride, lengths=lens[keep]), keep))
        same = np.array([i for i in keep if lens[i] == 64], np.int64)
        if len(same) == 0:
            same, width = keep[:1], int(lens[keep[0]])
        else:
            width = 64
        if width:
            a = aligned(len(same) * width + 16)[:len(same) * width]
            a[:] = np.frombuffer(b"".join(frames[i] for i in same), np.uint8)
            out.append(Layout("strided", a, np.arange(len(same), dtype=np.int64) * width,
                              lens[same], width, dict(stride=width), same))
    return out


def expected_buffer(host_data, offsets, lengths, fixed_frames):
    """The whole data array a correct fix-up leaves: every in-extent frame
    replaced by its fixed bytes, every other byte as it was."""
    want = np.array(host_data, np.uint8, copy=True)
    nb = len(want)
    for o, l, f in zip(offsets, lengths, fixed_frames):
        o, l = int(o), int(l)
        if l > MAX_FRAME or o > nb or l > nb - o:
            continue
        assert len(f) == l
        want[o:o + l] = np.frombuffer(f, np.uint8)
    return want


# ---------------------------------------------------------------- the comparer

def compare(buf, want, offsets, lengths, rep=None, want_rep=None, lo=0, what=""):
    """`buf`: the whole host buffer after the call, its bytes [lo, lo +
    len(want)) the batch's data and every other byte a guard (GUARD_FILL).
    Raises on the first differing byte, named as frame number, lane and offset
    in the frame, or as a gap / before data / after data; then on the first
    differing report row, field by field."""
    buf = np.asarray(buf, np.uint8)
    hi = lo + len(want)
    assert 0 <= lo and hi <= len(buf), (lo, hi, len(buf))
    offsets, lengths = np.asarray(offsets, np.int64), np.asarray(lengths, np.int64)
    if (buf[:lo] != GUARD_FILL).any():
        at = int(np.nonzero(buf[:lo] != GUARD_FILL)[0][-1])
        raise AssertionError(f"{what}: byte written before data: {lo - at} B ahead of it, now {buf[at]:#04x}")
    if (buf[hi:] != GUARD_FILL).any():
        at = int(np.nonzero(buf[hi:] != GUARD_FILL)[0][0])
        raise AssertionError(f"{what}: byte written after data: {at} B past its end, now {buf[hi + at]:#04x}")
    bad = np.nonzero(buf[lo:hi] != want)[0]
    if len(bad):
        p = int(bad[0])
        ok = (lengths <= MAX_FRAME) & (offsets <= len(want)) & (lengths <= len(want) - np.minimum(offsets, len(want)))
        order = np.argsort(offsets, kind="stable")
        order = order[ok[order]]
        j = int(np.searchsorted(offsets[order], p, side="right")) - 1
        i = int(order[j]) if j >= 0 else -1
        msg = f"{what}: {len(bad)} bytes differ; first at data byte {p}: got {buf[lo + p]:#04x}, want {want[p]:#04x}: "
        if i >= 0 and p < offsets[i] + lengths[i]:
            o, l = int(offsets[i]), int(lengths[i])
            msg += (f"frame {i} (lane {i % 256}) offset {p - o} of {l}, frame at data byte {o} (address parity {o & 1}"
                    f" within data)\ngot  {buf[lo + o:lo + o + min(l, 96)].tobytes().hex()}"
                    f"\nwant {want[o:o + min(l, 96)].tobytes().hex()}")
        elif i >= 0:
            msg += f"in the gap after frame {i} (lane {i % 256}), {p - int(offsets[i] + lengths[i])} B past its end"
        else:
            msg += "in the gap ahead of the first frame"
        raise AssertionError(msg)
    if rep is not None:
        assert rep.dtype == want_rep.dtype == abi.FIXUP_DTYPE, (rep.dtype, want_rep.dtype)
        assert rep.shape == want_rep.shape, (rep.shape, want_rep.shape)
        row64 = lambda a: np.ascontiguousarray(a).view(np.uint64)  # a nexg_fixup row is 8 B
        rows = np.nonzero(row64(rep) != row64(want_rep))[0]
        if len(rows):
            i = int(rows[0])
            diff = {n: (int(rep[i][n]), int(want_rep[i][n])) for n in rep.dtype.names if rep[i][n] != want_rep[i][n]}
            raise AssertionError(f"{what}: {len(rows)} report rows differ; first frame {i} (lane {i % 256}): "
                                 f"(got, want) {diff}")
