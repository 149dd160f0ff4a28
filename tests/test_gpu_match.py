"""GPU: the fixed-string match (nexg_match_batch) and the selection by its
rows (nexg_match_select) on the corpus of tests/match_frames.py.

The expectation is nex_amd.match.match_rows_host (pinned by the truth table
and the independent reference of tests/test_match_host.py) over the oracle's
records of each case, computed once per case and tiled to each count. Shapes:
every layout of helpers.layouts (the fuzz sets on the first only: the packed
batch from byte 1, where an occurrence starts on every address phase); the
counts around a wave and a 256-frame tile; the 65535-byte frame; for the
selection also 65793 frames, the scan's 256-tile carry. Every match call
checks that the two rows past out[count] keep their sentinel."""
import ctypes

import numpy as np
import pytest

from nex_amd import abi
from nex_amd import dns as hostdns
from nex_amd import match as M
from nex_amd import select as S
from nex_amd.engine import FrameBatch
from nex_amd.match import Pattern, PatternSet
from nex_amd.select import Filter, Rule
from tests import match_frames as mf
from tests.helpers import layouts, to_host

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
#: the cases tiled to every count
TILED = ("sweep L=5", "sweep L=16 frame", "header trap payload", "header trap frame", "windows", "nocase", "empty regions",
         "fuzz 7")
SENTINEL = 0xEE


def device_records(recs):
    import torch
    return torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).copy()).cuda()


def run_match(engine, batch, recs_dev, pset):
    """nexg_match_batch through the raw entry into a buffer with two rows to
    spare: the rows, after checking that the spare rows kept their sentinel."""
    import torch
    n = batch.count
    out = torch.full(((n + 2) * 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    pc = pset.to_c()
    fr = batch.to_c()
    rc = engine.lib.nexg_match_batch(engine.ctx, ctypes.byref(fr), None if recs_dev is None else ctypes.c_void_p(recs_dev.data_ptr()),
                                     ctypes.byref(pc), ctypes.c_void_p(out.data_ptr()), engine._stream(None))
    assert rc == abi.OK, engine.lib.nexg_ctx_last_error(engine.ctx)
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[n * 8:] == SENTINEL).all(), "a store past out[count]"
    return h[: n * 8].view(abi.MATCH_DTYPE)


def rows_equal(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("name", [c.name for c in mf.cases()])
def test_rows_equal_the_contract(engine, oracle, name):
    c = mf.case(name)
    recs, want = mf.expected(oracle, c)
    for lname, batch, keep in layouts(c.frames, only_first=not c.every_layout):
        k = slice(None) if keep is None else keep
        got = run_match(engine, batch, device_records(recs[k]), c.pset)
        rows_equal(got, want[k], f"{name}: {lname}")
        if c.pset.frame:  # the whole frame needs no records
            rows_equal(run_match(engine, batch, None, c.pset), want[k], f"{name}: {lname}, NULL records")


@pytest.mark.parametrize("count", COUNTS)
def test_counts_every_layout(engine, oracle, count):
    for name in TILED:
        c = mf.case(name)
        recs, want = mf.expected(oracle, c)
        which = np.arange(count) % len(c.frames)
        frames = [c.frames[i] for i in which]
        for lname, batch, keep in layouts(frames, only_first=not c.every_layout):
            w = which if keep is None else which[keep]
            got = run_match(engine, batch, device_records(recs[w]), c.pset)
            rows_equal(got, want[w], f"{name} n={count}: {lname}")


def test_engine_match_and_determinism(engine, oracle):
    import torch
    c = mf.case("fuzz 32")
    recs, want = mf.expected(oracle, c)
    batch = FrameBatch.from_packed(c.frames, pad_to=1)
    dev = device_records(recs)
    a = engine.match(batch, dev, c.pset)
    b = engine.match(batch, dev, c.pset)
    torch.cuda.synchronize()
    assert a.numel() == 8 * batch.count and torch.equal(a, b)
    rows_equal(to_host(a, abi.MATCH_DTYPE, batch.count), want, "Engine.match")
    assert len(set(want["mask"].tolist())) > 100  # many different rows: the accumulators are really shared
    with pytest.raises(ValueError):
        engine.match(batch, dev, PatternSet([]))
    empty = FrameBatch.from_packed([], pad_to=1)
    assert engine.match(empty, None, c.pset).numel() == 0


def table_of(batch):
    if batch.offsets is None:
        off = np.arange(batch.count, dtype=np.int64) * batch.stride
    else:
        off = batch.host_offsets()[: batch.count]
    return off, batch.frame_lengths()


SELECTIONS = [dict(), dict(any=0b1), dict(any=0b1100000), dict(all=0b11), dict(none=0b1), dict(any=0b110, none=0b1),
              dict(any=0b1, all=0b1000100), dict(all=0x80), dict(any=0xFFFFFFFF), dict(none=0xFFFFFFFF),
              dict(any=0x7F, all=0x7F, none=0x7F)]


@pytest.mark.parametrize("count", COUNTS + [65793])
def test_match_select_equals_the_host(engine, oracle, count):
    import torch
    c = mf.case("fuzz 7")
    _, rows = mf.expected(oracle, c)
    which = np.arange(count) % len(c.frames)
    frames = [c.frames[i] for i in which]
    hrows = rows[which]
    picked = set()
    for lname, batch, keep in layouts(frames, only_first=count > 1000):
        r = hrows if keep is None else hrows[keep]
        dev = torch.from_numpy(r.view(np.uint8).copy()).cuda() if len(r) else torch.zeros(8, dtype=torch.uint8, device="cuda")
        off, ln = table_of(batch)
        for kw in SELECTIONS:
            want = M.match_select_host(r, **kw)
            idx, sel = engine.match_select(batch, dev, **kw)
            what = (lname, count, kw)
            assert sel.count == len(want), what
            assert (to_host(idx, np.uint32, sel.count) == want).all(), what
            assert (to_host(sel.offsets, np.int64, sel.count) == off[want]).all(), what
            assert (to_host(sel.lengths, np.uint32, sel.count) == ln[want]).all(), what
            assert sel.data.data_ptr() == batch.data.data_ptr()
            assert bool(sel.hints & abi.FRAMES_MONOTONE) == (batch.offsets is None or batch.lengths is None)
            picked.add(len(want))
    if count >= 255:
        assert len(picked) > 4 and 0 in picked and count in picked  # none, all and several in between


def test_match_select_is_deterministic(engine, oracle):
    import torch
    c = mf.case("fuzz 7")
    recs, _ = mf.expected(oracle, c)
    which = np.arange(65793) % len(c.frames)
    batch = FrameBatch.from_packed([c.frames[i] for i in which], pad_to=1)
    rows = engine.match(batch, device_records(recs[which]), c.pset)
    runs = []
    for _ in range(2):
        idx, sel = engine.match_select(batch, rows, any=0b11, none=0b100)
        runs.append((idx.clone(), sel.offsets.clone(), sel.lengths.clone()))
    assert 0 < len(runs[0][0]) < 65793
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_select_match_dns_chain(engine, oracle):
    """select(udp port 53) -> gather_rows -> match on the selected table ->
    match_select -> dns on the result, against the same chain on the host."""
    from tests import dns_frames as df
    from nex_amd.frame import ParseOption
    cs = df.cycled(df.cases(), 700)
    frames = [c.frame for c in cs]
    batch = FrameBatch.from_packed(frames, pad_to=1)
    recs = engine.parse(batch, ParseOption(unwrap_vlan=True), out_kind=abi.OUT_RECORD)
    flt = Filter([Rule.udp() & Rule.port(53)])
    pset = CHAIN_SET
    # on the device
    idx, sel = engine.select(batch, recs, flt)
    rec_sel = engine.gather_rows(recs, 64, idx)
    rows = engine.match(sel, rec_sel, pset)
    idx2, sel2 = engine.match_select(sel, rows, any=0b11, none=0b100)
    rec_sel2 = engine.gather_rows(rec_sel, 64, idx2)
    dns, tile_first, entries, total = engine.dns(sel2, rec_sel2)
    # on the host
    hrecs = oracle.parse_frames(frames, abi.PARSE_VLAN)
    want_idx, want_idx2, finals = chain_host(frames, hrecs, flt, pset)
    assert 0 < len(want_idx2) < len(want_idx) < len(frames)
    assert (to_host(idx, np.uint32, sel.count) == want_idx).all()
    assert (to_host(rows, abi.MATCH_DTYPE, sel.count) ==
            M.match_rows_host([frames[i] for i in want_idx], hrecs[want_idx], [len(frames[i]) for i in want_idx], pset)).all()
    assert (to_host(idx2, np.uint32, sel2.count) == want_idx2).all()
    hdns = to_host(dns, abi.DNS_DTYPE, sel2.count)
    n_entries = 0
    for k, i in enumerate(finals):
        s, ent = hostdns.dns_frame_host(frames[i], hrecs[i])
        for f in s:
            assert int(hdns[f][k]) == s[f], (k, i, f)
        n_entries += len(ent)
    assert total == n_entries > 0


#: the chain's set: queries or answers for an A record in class IN, "example" in any case, and none with "org"
CHAIN_SET = PatternSet([Pattern(b"\x00\x01\x00\x01"), Pattern(b"EXAMPLE", nocase=True), Pattern(b"\x03org")])


def chain_host(frames, hrecs, flt, pset):
    """The chain's indices on the host: (selected by the filter, selected among those by the rows, the final frames)."""
    want_idx = S.select_host(frames, hrecs, [len(f) for f in frames], flt)[0]
    sub = [frames[i] for i in want_idx]
    rows = M.match_rows_host(sub, hrecs[want_idx], [len(f) for f in sub], pset)
    want_idx2 = M.match_select_host(rows, any=0b11, none=0b100)
    return want_idx, want_idx2, [int(want_idx[k]) for k in want_idx2]
