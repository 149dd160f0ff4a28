"""CPU: the far batch of tests/far_batch.py is what tests/test_gpu_far_batch.py
takes it to be. No 4-GiB array is made: the tables are arithmetic.

Anchors, per placement and boundary: the situation occurs (A: a short frame
begins 9 bytes below the boundary; B: one frame's last byte is boundary - 1 and
the next begins on it; C: the 65535-byte frame begins 30000 bytes below it);
the frames on 2^32 are not the first of a 256-frame group in the sparse or the
dense table; some group's base lies below 2^32 with members at or above it, so
that the member's u32 entry is below the base's low half and the subtraction
wraps; some group's base lies at or above 2^32; every offset lies within 2^32
after its group's base; and the u32 table of every form and view decodes to
the u64 offsets it was made from.

Strength: under each pass's host contract the frames of clusters 1 and 2 that
begin at or above their boundary are not trivial (at least 10 frames per
condition, the collision pair once), and
every filler's expected row is the trivial one. These are conditions on the
inputs; the GPU tests use the same objects."""
import numpy as np
import pytest

from nex_amd import abi
from nex_amd.match import NO_MATCH
from tests import far_batch as fb
from tests.far_batch import BOUNDARIES, BUFFER_BYTES, GIB2, GIB4, NO_BASES_BYTES

VIEWS = (BUFFER_BYTES, GIB4, NO_BASES_BYTES)


@pytest.fixture(scope="module")
def far():
    return fb.far()


@pytest.fixture(scope="module")
def exp(oracle):
    return fb.expect()


def tables(pl):
    """(name, offsets, rows of the frames that sit on each boundary) of the sparse and the dense table."""
    return (("forms 1-2", pl.off, pl.row), ("forms 3-4", pl.dense_off, {b: int(pl.dense_row[r]) for b, r in pl.row.items()}))


def test_corpus(far):
    lens = far.lengths[: far.K]
    assert 250 <= far.K <= 340
    assert (lens >= 2048).sum() == 1 and lens.max() == 65535
    assert {s.name for s in far.sections} == {"dns", "tunnel", "select", "flow", "match", "rewrite", "tcp options",
                                               "fix-up planted"}
    assert far.fillers[0] == 65535 and all(0 < n < 65535 for n in far.fillers[1:])
    for pl in far.placements.values():
        assert len(pl.ids) == 3 * far.K and 750 <= len(pl.ids) <= 1020
        for c in range(3):  # each cluster is the whole corpus, rotated
            assert sorted(pl.ids[c * far.K:(c + 1) * far.K].tolist()) == list(range(far.K))


@pytest.mark.parametrize("name", fb.PLACEMENTS)
def test_the_situation_occurs_at_both_boundaries(far, name):
    pl = far.placements[name]
    assert pl.start[0] == 1 and pl.bounds == BOUNDARIES
    for tname, off, rows in tables(pl):
        ln = np.diff(off) if tname == "forms 3-4" else pl.length
        assert (np.diff(off) >= 0).all()
        for b in BOUNDARIES:
            r = rows[b]
            o, n = int(off[r]), int(ln[r])
            if name == "A":  # the Ethernet header, and the aligned dword that covers the boundary, straddle it
                assert o == b - 9 and 14 <= n <= 64 and o < b < o + 14, (tname, b)
                assert far.frames[pl.wanted][12:14] == b"\x08\x00"
            elif name == "B":
                assert o == b and n > 0, (tname, b)
                assert int(off[r - 1]) + int(ln[r - 1]) == b and int(ln[r - 1]) > 0, (tname, b)
            else:  # the streamed sums and the match items cross it in the middle of the payload
                assert n == 65535 and o == b - 30000, (tname, b)
            # clusters on both sides of the boundary, frames back to back
            c = BOUNDARIES.index(b) + 1
            assert pl.start[c] < b < pl.end[c]
            k = slice(c * far.K, (c + 1) * far.K)
            assert (pl.off[k][1:] == pl.off[k][:-1] + pl.length[k][:-1]).all()
    # the clusters' 4-KiB margins never meet, and all of it lies inside the buffer
    assert pl.end[0] + 8192 < pl.start[1] and pl.end[1] + 8192 < pl.start[2] and pl.end[2] + 4096 <= BUFFER_BYTES


@pytest.mark.parametrize("name", fb.PLACEMENTS)
def test_group_anchors(far, name):
    pl = far.placements[name]
    for tname, off, rows in tables(pl):
        n = len(off)  # the entries of the u32 table (the sparse table's last slot repeats the last offset)
        if tname == "forms 1-2":
            off, n = np.concatenate([off, off[-1:]]), len(off) + 1
        r = rows[GIB4]
        crossing = [r, r - 1] if name == "B" else [r]
        for x in crossing:  # not the first of a group: its base is another frame's offset
            assert x % 256 != 0, (tname, x)
        base = off[(np.arange(n) >> 8) << 8]
        rel = off - base
        assert (rel >= 0).all() and (rel < GIB4).all(), tname  # every offset within 2^32 after its group's base
        if tname == "forms 3-4":  # a packed frame's end is completed from the frame's own group
            end_rel = off[1:] - base[:-1]
            assert (end_rel >= 0).all() and (end_rel < GIB4).all()
        wraps = (base < GIB4) & (off >= GIB4)
        assert wraps.any(), tname  # a base below 2^32 with members at or above it ...
        o32, b32 = (off & 0xFFFFFFFF)[wraps], (base & 0xFFFFFFFF)[wraps]
        assert (o32 < b32).all(), tname  # ... whose u32 entries are below the base's low half: o32 - (u32)base wraps
        assert (base >= GIB4).any(), tname  # a base at or above 2^32
        assert ((base < GIB2) & (off >= GIB2)).any() or (base[rows[GIB2]] < GIB2 <= off[rows[GIB2] + 1])


@pytest.mark.parametrize("name", [*fb.PLACEMENTS, "B1"])
def test_u32_tables_decode_to_their_offsets(far, name):
    pl = far.placements[name]
    for view in VIEWS:
        n = pl.rows_within(view)
        table, o = fb.table32(pl.off[:n], view, packed=False)
        assert len(table) == abi.offsets32_layout(n, view > 0xFFFFFFFF)[3]
        assert (abi.offsets32_decode(table, n, view) == o).all(), (name, view)
        if n < 3 * far.K:  # a cut view: the frames dropped are exactly those that do not fit
            assert pl.off[n] + pl.length[n] > view >= pl.off[n - 1] + pl.length[n - 1]
    table, o = fb.table32(pl.dense_off, BUFFER_BYTES, packed=True)
    count = len(pl.dense_off) - 1
    assert (abi.offsets32_decode(table, count, BUFFER_BYTES) == o).all(), name
    assert 65000 < count < 67000 and (count + 255) // 256 > 256  # the one-workgroup scans carry past 256 tiles


def test_views(far):
    """The buffer cut to 2^32 bytes still has bases; 0xFFFFFFFF bytes is the
    edge of the rule: no bases, and in B1 the last frame kept ends on the last
    data byte (in B the frame whose last byte is 0xFFFFFFFF is the first dropped)."""
    K = far.K
    b, b1 = far.placements["B"], far.placements["B1"]
    r = b.row[GIB4]
    assert b.rows_within(BUFFER_BYTES) == 3 * K
    assert b.rows_within(GIB4) == r and b.off[r - 1] + b.length[r - 1] == GIB4  # ends on the view's last byte
    assert b.rows_within(NO_BASES_BYTES) == r - 1
    r1 = b1.row[GIB4 - 1]
    assert r1 == r and b1.off[r1] == NO_BASES_BYTES
    assert b1.rows_within(NO_BASES_BYTES) == r1 and b1.off[r1 - 1] + b1.length[r1 - 1] == NO_BASES_BYTES
    assert (b1.ids == b.ids).all() and (b1.off[: 2 * K] == b.off[: 2 * K]).all()
    assert (b1.off[2 * K:] == b.off[2 * K:] - 1).all()
    for name in fb.PLACEMENTS:
        pl = far.placements[name]
        n = pl.rows_within(GIB4)
        assert 2 * K < n < 3 * K and n > 256 * 2  # part of cluster 2, more than two groups


@pytest.mark.parametrize("name", fb.PLACEMENTS)
def test_the_upper_clusters_are_not_trivial(far, exp, name):
    pl = far.placements[name]
    K = far.K
    flow = next(s for s in far.sections if s.name == "flow")
    pair_hash = int(exp.flows["hash"][flow.first + flow.count - 1])
    for c in (1, 2):
        rows = np.arange(c * K, (c + 1) * K)
        above = rows[pl.off[rows] >= BOUNDARIES[c - 1]]  # the frames that begin at or above the boundary
        assert len(above) >= K - 64 and len(rows) - len(above) >= 16, (name, c)
        for what, count in exp.strength(pl.ids[above]).items():
            assert count >= 10, (name, c, what, count)
        assert len(exp.keys_per_hash(pl.ids[above])[pair_hash]) >= 2, (name, c)  # the collision pair
    # the 65535-byte frame is valid UDP over IPv4 and carries the far pattern past byte 30000
    big = int(np.argmax(far.lengths[:K]))
    ok = abi.L_UDP | abi.L_IPV4 | abi.C_IP_OK | abi.C_L4_OK
    assert int(exp.recs["flags"][big]) & ok == ok and int(exp.recs["flags"][big]) >> abi.STATUS_SHIFT & 7 == 0
    far_bit = 1 << (len(fb.PATTERNS) - 1)
    for mode in (False, True):
        assert int(exp.match(mode)["mask"][big]) & far_bit
    assert far.frames[big].find(bytes(fb.PATTERNS[-1].data), 30000) > 30000


def test_every_filler_row_is_the_trivial_one(far, exp):
    """Each pass's row for a filler, from the 65535-byte zero frame (id K),
    is the trivial row; the shorter fillers have it too (but for the lengths
    in the record)."""
    K = far.K
    zero = slice(K, exp.n)
    assert far.frames[K] == bytes(65535) and exp.n - K == len(far.fillers)
    recs = exp.recs[zero]
    assert (recs["flags"] == abi.L_ETHERNET).all() and (recs["payload_off"] == 14).all()
    assert (recs["payload_len"] == far.lengths[zero] - 14).all() and (recs["packet_len"] == far.lengths[zero]).all()
    for n in abi.RECORD_DTYPE.names:
        if n not in ("flags", "payload_off", "payload_len", "packet_len", "l3_off"):
            assert not np.asarray(recs[n]).any(), n
    assert (exp.checksum(0xFFFFFFFF)[zero] == 0xFFFF).all() and (exp.checksum(5)[zero] == 0xFFFF).all()
    frames, rows = exp.fixup
    assert frames[K:] == far.frames[K:] and not rows[zero].view(np.uint8).any()
    for inc in (False, True):
        frames, rows, index = exp.rewrite(inc)
        assert frames[K:] == far.frames[K:] and (index[zero] == fb.NAT44).all()
        assert not rows["applied"][zero].any() and not rows["fixed"][zero].any() and (rows["action"][zero] == fb.NAT44).all()
    assert not exp.options[zero].view(np.uint8).any()
    tun, ioff, ilen = exp.tunnels
    assert (tun["kind"][zero] == abi.TUN_NONE).all() and not ioff[zero].any() and not ilen[zero].any()
    summaries, entries = exp.dns
    assert not summaries[zero].view(np.uint8).any() and all(len(e) == 0 for e in entries[K:])
    sel, rule = exp.select
    assert not sel[zero].any() and (rule[zero] == abi.RULE_NONE).all()
    assert tuple(exp.match_filler)[:3] == NO_MATCH
    for mode in (False, True):
        assert all(tuple(r)[:3] == NO_MATCH for r in exp.match(mode)[zero])
    assert not exp.flows[zero].view(np.uint8).any()
