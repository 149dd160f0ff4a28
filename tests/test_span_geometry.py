"""CPU: the span / two-pass geometry sweep (tests/span_geometry.py) checked
without a GPU: the constants it restates are the sources', every probe of
classes 1-3 sits at the position its case states (read from the offset table,
no exception), every geometry class has a case for each sub-tile size, the
generic-section groups decline and defer what they are meant to (counted by
the host harness, not by a restated predicate), the host harness and the oracle
agree on every packed batch, and the comparer reports seeded defects under the
right case name."""
import os
import re

import numpy as np
import pytest

from nex_amd import abi
from tests import helpers
from tests import span_geometry as sg
from tests.native import harness

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nex_amd", "csrc")
SUBS = sorted(set(sg.SPAN_SUB.values()))
LAYOUTS = [(s, 0) for s in sg.SHIFTS] + [(0, 16)]


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_constants_are_the_sources():
    parse, kern, core = _src("nexg_parse.hip"), _src("parse_kernels.hpp"), _src("frame_core.hpp")
    assert int(re.search(r"#define NEXG_SPAN_SUB (\d+)", parse).group(1)) == sg.SPAN_SUB["other"]
    assert f"k_parse_span<OUT, {sg.SPAN_SUB['record']}, 1>" in parse
    assert int(re.search(r"#define NEXG_SPAN_SLOT (\d+)", core).group(1)) == sg.SLOT
    assert int(re.search(r"constexpr uint32_t kDefer = (\d+);", core).group(1)) == sg.K_DEFER
    m = re.search(r"constexpr uint32_t kApron = NEXG_SPAN_SLOT > (\d+) \? NEXG_SPAN_SLOT : (\d+);", kern)
    assert int(m.group(1)) == int(m.group(2)) == sg.APRON >= sg.SLOT
    assert int(re.search(r"constexpr uint32_t kLaneWin = (\d+);", kern).group(1)) == sg.LANE_WIN
    assert int(re.search(r"constexpr uint32_t kPiece = (\d+);", kern).group(1)) == sg.K_PIECE
    assert int(re.search(r"constexpr uint32_t kTile = (\d+);", kern).group(1)) == sg.TILE
    assert int(re.search(r"constexpr uint32_t kBuckets = (\d+);", kern).group(1)) == sg.BUCKETS
    assert sg.WIN == sg.SLOT + 4  # NW = kSlot / 4 + 1 dwords


def _lengths(lay):
    return np.array([len(f) for f in lay.frames], np.int64)


def check_positions(lay, sub):
    """Every case of classes 1-3 at its stated position, from the table."""
    offs, lens = np.array(lay.offs, np.int64), _lengths(lay)
    assert lay.cases
    for c in lay.cases:
        assert c.sub == sub and c.k >= 1, c
        if c.what == "hi":  # the group's last byte
            g0 = c.index // sg.TILE * sg.TILE
            last = min(g0 + sg.TILE, lay.n) - 1
            hi = int(offs[last] + lens[last]) - (int(offs[g0]) & ~15)
            assert hi == int((offs[g0:last + 1] + lens[g0:last + 1]).max()) - (int(offs[g0]) & ~15)
            assert hi == c.k * sub + c.d, (sg.case_name(c), hi)
            assert sg.position(c, offs, lens, lay.frames) == hi, sg.case_name(c)
        else:
            assert sg.position(c, offs, lens, lay.frames) == c.k * sub + c.d, sg.case_name(c)


def agree(oracle, lay, flags=0, ip_offset=0, what=""):
    """The oracle's records of a layout; on a packed one the host harness's
    span emulation must give the same."""
    data, offs, lens = lay.table()
    want = oracle.parse_packed(data, offs, lens, flags=flags, ip_offset=ip_offset)
    if lens is None:
        helpers.records_equal(harness.span_groups(data, offs, flags, ip_offset), want, lay.frames, f"harness {what}")
    return want


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("shift,gap", LAYOUTS)
def test_classes_1_to_3(oracle, sub, shift, gap):
    lay = sg.class123(sub, shift, gap)
    assert lay.offs[0] == shift + gap
    check_positions(lay, sub)
    for name, pred in sg.GEOMETRY_CLASSES.items():
        assert pred(lay, sub), (name, sub, shift, gap)
    want = agree(oracle, lay, what=f"SUB {sub} shift {shift} gap {gap}")
    # both verdicts occur on the probes, and every filler is checksum-valid
    probes = np.array(sorted({c.index for c in lay.cases}))
    l4 = (want["flags"][probes] & abi.C_L4_OK) != 0
    assert l4.any() and (~l4).any()
    fill = np.setdiff1d(np.arange(lay.n), probes)
    fill = fill[_lengths(lay)[fill] >= sg.MIN_FILL]
    ok = abi.C_L4_OK | abi.C_IP_OK
    assert ((want["flags"][fill] & ok) == ok).all()
    if shift == 0 and gap == 0:
        for flags, ipo in ((abi.PARSE_STRICT, 0), (abi.PARSE_FROM_IP, 14), (abi.PARSE_VLAN, 0)):
            agree(oracle, lay, flags, ipo, f"SUB {sub} flags {flags}")


def test_probe_list():
    p = sg.probes()
    need = ["udp4_200", "tcp6_ts_300", "udp4_60", "udp4_81", "pad64", "pad_ip83_180", "pad_ip84_180", "pad_ip85_180",
            "pad_ip120_180", "tcp4_ipopt_400", "udp6_ext2_150", "arp42", "len0", "len1", "len13", "vlan_tagged_pad",
            "vlan_untagged_pad"]
    assert set(need) <= set(p)
    assert [len(p[n]) for n in ("len0", "len1", "len13", "arp42", "pad64")] == [0, 1, 13, 42, 64]
    for n in need:
        assert (n + "_bad" in p) == (len(p[n]) > 80), n
    for n, e in (("pad_ip83_180", 83), ("pad_ip84_180", 84), ("pad_ip85_180", 85), ("pad_ip120_180", 120), ("pad64", 50)):
        assert sg.ip_end_of(p[n]) == e
    for n in ("vlan_tagged_pad", "vlan_untagged_pad"):  # over 64 B between byte 80 and the IP end
        assert len(p[n]) == 230 and (p[n][12:14] == b"\x81\x00") == (n == "vlan_tagged_pad")
    assert sg.ip_end_of(p["vlan_untagged_pad"]) - 80 > sg.K_DEFER


@pytest.mark.parametrize("sub", SUBS)
def test_span_end_batches(oracle, sub):
    lays = sg.span_end_batches(sub)
    counts = set()
    for lay in lays:
        data, offs, lens = lay.table()
        assert lens is None and len(data) == int(offs[-1]) == lay.pos  # the data ends at hi
        check_positions(lay, sub)
        agree(oracle, lay, what=f"span end {lay.cases}")
        counts.add(lay.n % sg.TILE)
    assert counts >= set(sg.PARTIAL_COUNTS) | {0}
    have = {(c.probe, c.d) for lay in lays for c in lay.cases}
    for name in ("udp4_200", "udp4_60", "len0", "udp4_single"):
        assert {(name, e) for e in sg.END_EPS} <= have, name


@pytest.mark.parametrize("shift", [0, 1])
def test_prefix_wrap(oracle, shift):
    lay = sg.prefix_wrap(shift)
    data, offs, _ = lay.table()
    assert int(offs[0]) % 2 == shift and sum(len(f) == 65535 for f in lay.frames) == 8 and lay.n <= sg.TILE
    assert sg.prefix_wraps(data, offs)  # the sum passes 2^32 inside some frame's [80, len)
    assert all(len(lay.frames[i]) == 65535 for i in sg.prefix_wraps(data, offs))
    want = agree(oracle, lay, what="prefix wrap")
    ok = abi.C_L4_OK | abi.C_IP_OK
    assert ((want["flags"] & ok) == ok).all()


def test_generic_section_groups(oracle):
    """The declined sets, from the harness's declined flags."""
    seen = set()
    for name, frames, lanes in sg.generic_groups():
        lay = sg.packed(frames, 4)
        data, offs, _ = lay.table()
        (recs, declined, st), = harness.span_group_stats(data, offs)
        assert np.nonzero(declined)[0].tolist() == lanes, name
        assert st["declined"] == len(lanes), name
        helpers.records_equal(recs, oracle.parse_packed(data, offs, None), frames, name)
        buckets = [sg.span_bucket(frames[t]) for t in lanes]
        seen.add((len(lanes), len(set(buckets))))
        if len(lanes) == 1:
            seen.add(("lane", lanes[0]))
        if lanes == list(range(64, 128)):
            seen.add("wave")
    assert {("lane", 0), ("lane", 63), ("lane", 64), ("lane", 255), "wave", (256, 1), (256, sg.BUCKETS)} <= seen
    assert {n for n, _ in (s for s in seen if isinstance(s, tuple) and s[0] != "lane")} >= {1, 4, 5, 64, 256}
    assert sorted(sg.span_bucket(f) for f in sg.declined_pool()) == list(range(sg.BUCKETS))


def test_deferred_range_groups(oracle):
    """Worker waves with 1, 3, 4, 5, 8 and 64 deferred ranges, counted by
    harness_span_stats; every range length and every start phase mod 16."""
    counts, lengths, phases = [], set(), set()
    for name, frames, lanes in sg.deferred_groups():
        lay = sg.packed(frames)
        data, offs, _ = lay.table()
        (recs, declined, st), = harness.span_group_stats(data, offs, abi.PARSE_VLAN)
        assert np.nonzero(declined)[0].tolist() == lanes and st["declined"] <= 64, name  # one worker wave
        assert st["deferred"] == len(lanes), (name, st)
        counts.append(st["deferred"])
        helpers.records_equal(recs, oracle.parse_packed(data, offs, None, flags=abi.PARSE_VLAN), frames, name)
        for t in lanes:
            f = frames[t]
            l3 = 18 if f[12:14] == b"\x81\x00" else 14
            lengths.add(l3 + int.from_bytes(f[l3 + 2: l3 + 4], "big") - 80)
            phases.add((int(offs[t]) + 80) % 16)
    assert counts == list(sg.WAVE_DEFERRED)
    assert lengths == set(sg.RANGE_LENGTHS) and min(lengths) == sg.K_DEFER + 1
    assert phases == set(range(16))


def test_stride200_crosses_edges():
    arr = sg.stride200()
    assert arr.shape[1] == 200 and arr.shape[0] > 3 * sg.TILE
    for sub in SUBS:  # a frame of some group straddles an edge of each sub-tile size
        assert any(200 * i < sub < 200 * (i + 1) for i in range(sg.TILE))


def test_two_pass_batch(oracle):
    data, offs, lens, notes = sg.two_pass_batch()
    assert len(offs) % 64 == 0
    what = dict(notes)
    pieces = sg.two_pass_pieces(offs, lens)
    totals = [pieces[w] for w, n in notes if n.startswith("piece total")]
    assert totals == list(sg.PIECE_TOTALS) and any(t % 4 for t in totals) and 0 in totals
    # wave bases: the lowest tail start of every wave with a tail, rounded down to 256
    ts, te = offs.astype(np.int64) + 80, (offs + lens).astype(np.int64)
    tail = lens > sg.LANE_WIN
    edges = set()
    for w, n in notes:
        s = slice(64 * w, 64 * w + 64)
        if n == "range edges":
            base = ts[s][tail[s]].min() // 256 * 256
            for a, b in zip(ts[s][tail[s]] - base, te[s][tail[s]] - base):
                for m in (256, 16):
                    edges |= {("start", m, (a + 1) % m - 1), ("end", m, (b + 1) % m - 1)}
        if n == "tail lengths":
            assert set(sg.TAIL_LENGTHS) <= set((te[s] - ts[s])[tail[s]].tolist())
        if n.startswith("long frame at lane"):
            lane = int(n.split()[-1])
            assert lens[s][lane] == 65535 and (np.delete(lens[s], lane) < 200).all()
        if n == "decreasing addresses":
            assert (np.diff(offs[s].astype(np.int64)) < 0).all()
        if n == "duplicate rows":
            assert (offs[s][0::2] == offs[s][1::2]).all() and (lens[s] > sg.LANE_WIN).all()
    assert {(k, m, d) for k in ("start", "end") for m in (256, 16) for d in (-1, 0, 1)} <= edges
    assert {"range edges", "tail lengths", "decreasing addresses", "duplicate rows"} <= set(what.values())
    want = oracle.parse_packed(data, offs, lens)
    ok = abi.C_L4_OK | abi.C_IP_OK
    assert ((want["flags"][lens >= sg.MIN_FILL] & ok) == ok).all()
    # the lane-window emulation of the host harness (k_parse_lane80's fast path + the generic core)
    helpers.records_equal(harness.parse_packed(data, offs, lens, use_fast=4), want, None, "two-pass harness")
    ends = sg.window_end_batches()
    assert sorted(int(o[-1]) % 16 for _, o, _ in ends) == list(range(16))
    for d, o, n in ends:
        assert len(d) == int(o[-1] + n[-1]) and len(d) - int(o[-1]) < sg.WIN


def test_comparer_reports_seeded_defects(oracle):
    sub = SUBS[0]
    lay = sg.Layout(sub)
    sg.head_sweep(lay, ["udp4_200", "tcp4_ipopt_400"])
    data, offs, _ = lay.table()
    want = oracle.parse_packed(data, offs, None)
    lens = np.array([len(f) for f in lay.frames], np.int64)
    for kind in (abi.OUT_RECORD, abi.OUT_DESC, abi.OUT_FLAGS, abi.OUT_VERDICT):
        sg.compare(kind, sg.host_buffer(kind, want), want, lens, lay.cases, "clean")
    c = lay.cases[150]

    def report(kind, seed):
        buf = sg.host_buffer(kind, want)
        seed(buf)
        with pytest.raises(AssertionError) as e:
            sg.compare(kind, buf, want, lens, lay.cases, "seeded")
        return str(e.value)

    def verdict_bit(itemsize):
        def seed(buf):
            at = sg.GUARD + c.index * itemsize
            word = int.from_bytes(buf[at: at + 2].tobytes(), "little") ^ abi.C_L4_OK
            buf[at: at + 2] = np.frombuffer(word.to_bytes(2, "little"), np.uint8)
        return seed

    assert abi.C_L4_OK < 1 << 16
    for kind, size, field in ((abi.OUT_RECORD, 64, "flags"), (abi.OUT_DESC, 8, "flags"), (abi.OUT_FLAGS, 4, "flags"),
                              (abi.OUT_VERDICT, 2, "verdict")):
        msg = report(kind, verdict_bit(size))
        assert sg.case_name(c) in msg and f"first differing field {field}" in msg, msg
    assert abi.RECORD_DTYPE.names[0] == "flags"

    def csum(buf):
        at = sg.GUARD + c.index * 64 + abi.RECORD_DTYPE.fields["l4_csum_calc"][1]
        buf[at] ^= 0x01
    msg = report(abi.OUT_RECORD, csum)
    assert sg.case_name(c) in msg and "first differing field l4_csum_calc" in msg, msg
    assert f"SUB {sub}" in msg and f"k={c.k}" in msg and f"d={c.d}" in msg and c.probe in msg

    def guard_lo(buf):
        buf[sg.GUARD - 1] ^= 0xFF

    def guard_hi(buf):
        buf[-sg.GUARD] ^= 0xFF
    assert f"guard byte {sg.GUARD - 1} before" in report(abi.OUT_RECORD, guard_lo)
    assert "guard byte 0 after" in report(abi.OUT_FLAGS, guard_hi)
    # a frame that is no probe is named by the case in front of it
    filler = c.index + 1
    assert filler not in {x.index for x in lay.cases}

    def filler_flags(buf):
        buf[sg.GUARD + filler * 4] ^= 0x01
    msg = report(abi.OUT_FLAGS, filler_flags)
    assert f"frame {filler} (behind {sg.case_name(c)})" in msg, msg
