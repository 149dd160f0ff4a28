"""CPU: the builder sweep's grid, corpus and comparer (tests/builder_sweep.py),
checked without a GPU: every dispatch class of the builders' launchers is
reached at every count, the oracle's frames carry the checksum edges and agree
with an independent Internet checksum, and the comparer reports every seeded
defect."""
import collections

import numpy as np
import pytest

from tests import builder_sweep as bs
from tests import helpers


@pytest.fixture(scope="module")
def grid(oracle):
    """[(case, inputs, oracle frames)] of the whole grid, built once."""
    out = []
    for seed, c in enumerate(bs.cases()):
        inp = bs.inputs(c, seed, oracle)
        out.append((c, inp, bs.expected(oracle, c, inp)))
    return out


def test_every_class_at_every_count():
    seen = collections.Counter()
    for c in bs.cases():
        hits = [name for name, _, pred in bs.DISPATCH_CLASSES if pred(c)]
        assert len(hits) == 1, (c, hits)
        seen[hits[0], c.count] += 1
        seen[hits[0], c.count, c.out_shift % 16 == 0] += 1
    for name, gap, _ in bs.DISPATCH_CLASSES:
        for n in bs.COUNTS:
            assert seen[name, n], (name, n)
            if gap == bs.FILL:  # the direct kernels: an unaligned out at any stride, an aligned one past 128 B
                assert seen[name, n, True] and seen[name, n, False], (name, n)
    assert len({name for name, _, _ in bs.DISPATCH_CLASSES}) == len(bs.DISPATCH_CLASSES)


def test_grid_edges_present():
    cs = bs.cases()
    for b in ("udp4", "udp4_tuples", "udp6", "tcp", "icmp"):
        mine = [c for c in cs if c.builder == b]
        assert {0, 1, 2, 3, 4, 5, 63, 64, 65, 66, 300, 515} <= {c.payload_len for c in mine}, b
        for sh in (0, 1, 2, 3):
            assert {1, 3, 4, 61, 63, 64} <= {c.payload_len for c in mine if c.pay_shift == sh}, (b, sh)
        assert all(c.count <= 513 for c in mine)
    for b, fam in (("udp4", 4), ("udp6", 6), ("tcp", 4), ("tcp", 6)):
        big = [c for c in cs if c.builder == b and c.family == fam and c.payload_len == bs.max_payload(b, fam)]
        assert big and all(c.count == 257 for c in big), (b, fam)
    assert {c.options for c in cs if c.builder == "tcp"} == set(bs.TCP_OPTIONS)
    lane = {c.out_stride for c in cs if c.builder == "icmp" and c.family == 4 and c.form == "probe"}
    assert {43, 44, 48, 49, 63, 64, 68, 69, 96, 97} <= lane
    # the optional arrays pairwise: every pair of names in all four presence combinations
    for b, names in bs.OPTIONAL.items():
        have = {c.arrays for c in cs if c.builder == b}
        for x in names:
            for y in names:
                if x < y:
                    combos = {(x in a, y in a) for a in have}
                    assert len(combos) == 4, (b, x, y)


def test_expected_is_the_single_frame_builders(oracle, grid):
    """builder_sweep.expected (oracle.build_rows_batch) row by row against the
    oracle's single-frame entries called one at a time, on a case of every
    builder, family and form."""
    seen = set()
    for c, inp, want in grid:
        key = (c.builder, c.family, c.form, bool(c.options), c.payload_len > 0)
        if key in seen or c.count != 257 or c.payload_len > 600:
            continue
        seen.add(key)
        r, k, pay = inp["rows"], inp["const"], inp["payload"]
        for i in (0, 1, 63, 64, 255, 256):
            dmac = bytes(r["dst_mac"][i])
            if "multicast" in c.arrays:
                dmac = b"\x33\x33" + bytes(r["dst"][i, 12:16])
            spec = oracle.ip_spec(c.family, bytes(r["src"][i]), bytes(r["dst"][i]), bytes(r["src_mac"][i]), dmac,
                                  int(r["ip_id"][i]), k["ttl"], k["ip_flags"], k["tos"], k["flow_label"])
            u32 = lambda a: int.from_bytes(bytes(a), "big")
            if c.builder in ("udp4", "udp4_tuples"):
                one = oracle.build_udp4(bytes(r["src_mac"][i]), dmac, u32(r["src"][i]), u32(r["dst"][i]), int(r["p0"][i]),
                                        int(r["p1"][i]), int(r["ip_id"][i]), k["ttl"], k["ip_flags"], k["tos"], pay)
            elif c.builder == "udp6":
                one = oracle.build_udp6(bytes(r["src_mac"][i]), dmac, bytes(r["src"][i]), bytes(r["dst"][i]),
                                        int(r["p0"][i]), int(r["p1"][i]), k["ttl"], k["tos"], k["flow_label"], pay)
            elif c.builder == "tcp":
                one = oracle.build_tcp(spec, int(r["p0"][i]), int(r["p1"][i]), int(r["seq"][i]), int(r["ack"][i]),
                                       k["tcp_flags"], k["window"], k["urg"], c.options, pay)
            elif c.builder == "icmp":
                one = oracle.build_icmp_echo(spec, k["icmp_type"], k["icmp_code"], int(r["p0"][i]), int(r["p1"][i]), pay)
            elif c.builder == "arp":
                one = oracle.build_arp(dmac, bytes(r["src_mac"][i]), bytes(r["src"][i]), bytes(r["target_mac"][i]),
                                       bytes(r["dst"][i]), operation=k["arp_operation"])
            else:
                one = oracle.build_ndp_ns(spec)
            assert want[i].tobytes() == one, (c, i)
    assert {b for b, *_ in seen} == set(bs.BUILDERS) and len(seen) >= 20


def be16(frames, off):
    return (frames[:, off].astype(np.uint32) << 8) | frames[:, off + 1]


def test_checksum_edges_in_corpus(grid):
    """Every checksum-bearing builder and family meets a computed zero: the
    oracle keeps the complement of a folded 0xFFFF, 0x0000, with no
    substitution of 0xFFFF (Q18 for UDP; the same finalize for the others), and
    emits 0xFFFF only for an all-zero message (ICMP over IPv4)."""
    l4 = collections.defaultdict(set)
    ip = collections.defaultdict(set)
    for c, inp, want in grid:
        for row, which, target in inp["solved"]:
            ck = int(be16(want[row: row + 1], bs.checksum_offset(c, which))[0])
            if target in (0x0000, 0xFFFF):
                allzero = (which == bs.L4_CK and c.builder == "icmp" and c.family == 4 and
                           not (want[row, 34:36].any() or want[row, 38:].any()))
                assert ck == (0xFFFF if allzero else 0x0000), (c, row, which, hex(ck))
            else:
                assert ck == target, (c, row, which, hex(ck))
        off = bs.checksum_offset(c, bs.L4_CK)
        if off is not None:
            l4[c.builder, c.family] |= set(np.unique(be16(want, off)).tolist()) & {0x0000, 0xFFFF, 0x0001}
        if bs.checksum_offset(c, bs.IP_CK) is not None:
            ip[c.builder] |= set(np.unique(be16(want, 24)).tolist()) & {0x0000, 0xFFFF, 0x0001}
    for b in ("udp4", "udp4_tuples", "udp6", "tcp", "icmp", "ndp_ns"):
        for fam in bs._families(b):
            assert {0x0000, 0x0001} <= l4[b, fam], (b, fam, l4[b, fam])
    assert 0xFFFF in l4["icmp", 4]  # the all-zero echo reply
    for b in ("udp4", "udp4_tuples", "tcp", "icmp"):
        assert {0x0000, 0x0001} <= ip[b], (b, ip[b])
        assert 0xFFFF not in ip[b]  # a header starting 0x45 never sums to zero


def csum_rows(m):
    """RFC 1071 over every row of an (n, k) uint8 matrix (independent of the oracle)."""
    if m.shape[1] % 2:
        m = np.concatenate([m, np.zeros((m.shape[0], 1), np.uint8)], axis=1)
    s = np.ascontiguousarray(m).view(">u2").astype(np.uint64).sum(axis=1)
    for _ in range(4):
        s = (s & 0xFFFF) + (s >> 16)
    return (~s & 0xFFFF).astype(np.uint32)


def checksum_inputs(c, want):
    """[(stored checksum per frame, bytes summed per frame with the field zero)]:
    the IPv4 header, and the L4 segment behind its pseudo-header."""
    n, out = want.shape[0], []
    if bs.checksum_offset(c, bs.IP_CK) is not None:
        h = want[:, 14:34].copy()
        h[:, 10:12] = 0
        out.append((be16(want, 24), h))
    off = bs.checksum_offset(c, bs.L4_CK)
    if off is not None:
        v4 = want[0, 12] == 0x08
        l4 = 34 if v4 else 54
        proto = int(want[0, 23 if v4 else 20])
        seg = want[:, l4:].copy()
        seg[:, off - l4: off - l4 + 2] = 0
        if proto == 1:  # ICMP over IPv4 sums the message alone
            out.append((be16(want, off), seg))
        else:
            ln = seg.shape[1]
            tail = np.broadcast_to(np.array([0, proto, ln >> 8, ln & 0xFF], np.uint8), (n, 4))
            addrs = want[:, 26:34] if v4 else want[:, 22:54]
            if not v4:  # RFC 8200: 32-bit length and next header; the same sum
                tail = np.broadcast_to(np.array([ln >> 24, (ln >> 16) & 0xFF, (ln >> 8) & 0xFF, ln & 0xFF, 0, 0, 0, proto],
                                                np.uint8), (n, 8))
            out.append((be16(want, off), np.concatenate([addrs, tail, seg], axis=1)))
    return out


def test_oracle_agrees_with_independent_checksum(grid):
    """The oracle's stored checksums equal RFC 1071 over the header, and over
    the pseudo-header and segment, of its own frames, with no allowance beyond
    Q18: where the sum complements to 0 the oracle's UDP builders store 0 (they
    do not substitute 0xFFFF), which is what the plain RFC 1071 value is too.
    Every frame through the vectorised sum; the planted and solved rows also
    through helpers.rfc1071."""
    rng = np.random.default_rng(5)
    probe = rng.integers(0, 256, (64, 37), dtype=np.uint8)
    assert csum_rows(probe).tolist() == [helpers.rfc1071(bytes(r)) for r in probe]
    for c, inp, want in grid:
        rows = sorted({0, c.count - 1} | {r for r, _, _ in inp["solved"]})
        for stored, data in checksum_inputs(c, want):
            calc = csum_rows(data)
            bad = np.nonzero(calc != stored)[0]
            assert bad.size == 0, (c, int(bad[0]), hex(int(calc[bad[0]])), hex(int(stored[bad[0]])))
            if data.shape[1] < 2048:
                for r in rows:
                    assert helpers.rfc1071(bytes(data[r])) == int(stored[r]), (c, r)


def pick(grid, pred):
    return next((c, inp, want) for c, inp, want in grid if pred(c, inp, want))


def seeded(c, want, edit):
    name, gap = bs.classify(c)
    buf = bs.layout(c, want, gap)
    bs.compare(c, buf, want)  # unmodified bytes pass
    lo = bs.GUARD + c.out_shift
    edit(buf, lo)
    with pytest.raises(AssertionError) as e:
        bs.compare(c, buf, want)
    return str(e.value), name


def test_comparer_reports_seeded_defects(grid):
    ragged = lambda c, *_: c.count == 513 and c.builder == "tcp" and c.out_shift == 0
    # one byte flipped in the last frame of a ragged tile
    c, inp, want = pick(grid, ragged)
    L, S, n = bs.frame_len(c), c.out_stride, c.count

    def flip(buf, lo):
        buf[lo + (n - 1) * S + L - 1] ^= 0x10
    msg, name = seeded(c, want, flip)
    assert f"frame {n - 1} (lane {(n - 1) % 256})" in msg and f"offset {L - 1}" in msg and name in msg
    assert want[n - 1].tobytes().hex() in msg and str(c) in msg
    # a checksum off by one end-around carry
    off = bs.checksum_offset(c, bs.L4_CK)

    def carry(buf, lo):
        v = ((int(buf[lo + 300 * S + off]) << 8 | int(buf[lo + 300 * S + off + 1])) + 1) & 0xFFFF
        buf[lo + 300 * S + off: lo + 300 * S + off + 2] = (v >> 8, v & 0xFF)
    msg, _ = seeded(c, want, carry)
    assert "frame 300 (lane 44)" in msg
    # a 0xFFFF checksum replaced by 0x0000
    c, inp, want = pick(grid, lambda c, inp, w: c.builder == "icmp" and c.family == 4 and c.count > 1 and
                        (be16(w, 36) == 0xFFFF).any())
    i = int(np.nonzero(be16(want, 36) == 0xFFFF)[0][-1])

    def zero_ck(buf, lo):
        buf[lo + i * c.out_stride + 36: lo + i * c.out_stride + 38] = 0
    msg, _ = seeded(c, want, zero_ck)
    assert f"frame {i} " in msg and "offset 36" in msg
    # one non-zero byte in a gap that must be zero, one zero byte in a gap that must stay as it was; and for
    # both kinds of class one byte written in the trailing guard and in the leading one
    for want_gap in (0, bs.FILL):
        c, inp, want = pick(grid, lambda c, *_: c.count == 257 and c.out_stride > bs.frame_len(c) + 1 and
                            bs.classify(c)[1] == want_gap)
        L, S = bs.frame_len(c), c.out_stride

        def gap_byte(buf, lo):
            buf[lo + 256 * S + S - 1] = 1 if want_gap == 0 else 0
        msg, _ = seeded(c, want, gap_byte)
        assert "gap" in msg and "frame 256 (lane 0)" in msg and f"offset {S - 1}" in msg

        def trailing(buf, lo):
            buf[lo + c.count * S] = 0
        msg, _ = seeded(c, want, trailing)
        assert "after out" in msg

        def leading(buf, lo):
            buf[lo - 1] = 0
        msg, _ = seeded(c, want, leading)
        assert "before out" in msg
    # one frame's payload rotated by one byte
    c, inp, want = pick(grid, lambda c, *_: c.builder == "udp6" and c.payload_len == 63 and c.count == 257)
    S = c.out_stride

    def rotate(buf, lo):
        p = buf[lo + 255 * S + 62: lo + 255 * S + 62 + 63].copy()
        buf[lo + 255 * S + 62: lo + 255 * S + 62 + 63] = np.roll(p, 1)
    msg, _ = seeded(c, want, rotate)
    assert "frame 255 (lane 255)" in msg


def test_knob_classes_cover_the_measurement_instances():
    """Under each setting of the measurement library the probe cases reach the
    instances no product dispatch reaches: k_build_probe at kch 3 and for ICMP,
    k_build_lane for TCP, the one-wave k_build_probe."""
    names = collections.defaultdict(set)
    for c in bs.cases():
        for s in bs.KNOB_SETTINGS:
            k = bs.knob_class(c, s)
            if k:
                names[s].add(k[0])
    assert {"k_build_probe<1,3,4> icmp4", "k_build_probe<4,4,4> icmp6", "k_build_probe<4,5,4> icmp6"} \
        <= names["NEXG_PROBE_ICMP=1"]
    assert {"k_build_l4<4,icmp,64,probe>", "k_build_l4<4,icmp,80,probe>"} <= names["NEXG_PROBE_ICMP=2"]
    assert {"k_build_lane<4,tcp,68,64>", "k_build_lane<4,tcp,96>", "k_build_lane<6,tcp,96>"} \
        <= names["NEXG_PROBE_LANE_TCP=1"]
    assert {"k_build_probe<1,4,1> tcp4", "k_build_probe<4,5,1> tcp6", "k_build_probe<4,4,1> udp6",
            "k_build_probe<4,8,1> udp6"} <= names["NEXG_PROBE_WAVES=1"]
