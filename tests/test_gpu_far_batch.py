"""GPU: every pass on batches whose frame offsets cross 2^31 and 2^32
(tests/far_batch.py: one corpus placed at byte 1, around 2^31 and around 2^32
of a device buffer of 2^32 + 2 MiB zero bytes; three placements A / B / C of
what sits on the boundaries, and B1 for the largest batch without group bases).

What runs here and nowhere else: table_extent / table_off with group bases
(u32 offsets over 4 GiB, packed and beside lengths), frame_extent's u32 +
lengths branch over 4 GiB, every kernel's address arithmetic after the extent
with an offset at or above 2^32 (match, select's IPv6 address reads, decap,
rewrite's header window, the fix-up, DNS, the option decode, the checksum, the
flow groups' and the flow table's key compares), and the 64-bit outputs
(decap's inner_off, the selections' out_off, the gather plan's offsets and the
gather copy's chunk index) with values at and above 2^32.

Every expectation is the pass's host contract over the frames (far_batch.Expect,
one row per distinct frame) taken at the table's ids; no device result on a
near batch is one. All comparisons are exact. Every per-frame output and every
selection's outputs are written through the raw entry into buffers with two
sentinel rows past `count`. The in-place passes compare the clusters' bytes with
4 KiB on each side, check with reductions on the device that every other byte of
the buffer is still zero, and put the clusters back.

The tables (far_batch's forms): 1 u64 offsets + lengths, with and without
FRAMES_MONOTONE; 2 its u32 table; both also on the buffer cut to 2^32 bytes
(bases, but every offset below 2^32) and, for B and B1, to 0xFFFFFFFF bytes
(no bases); 3 the dense packed table with about 65.5k filler frames (66.5k rows, 260
tiles); 4 its u32 table."""
import ctypes
from collections import namedtuple

import numpy as np
import pytest

from nex_amd import abi
from nex_amd.engine import FlowTable, FrameBatch
from nex_amd.flow import groups_host, merge_host, partition_host, sort_host
from nex_amd.frame import ParseMode, ParseOption
from nex_amd.match import match_select_host
from nex_amd.rewrite import rewrite_host
from tests import far_batch as fb
from tests import flow_table_ref as tr
from tests import helpers
from tests.far_batch import BUFFER_BYTES, FIX_OPTION, GIB4, NO_BASES_BYTES
from tests.helpers import to_host

pytestmark = pytest.mark.gpu

SENTINEL = 0xEE
MARGIN = 4096
VLAN = ParseOption(unwrap_vlan=True)
FROM_IP = ParseOption(from_ip_packet=True, offset=0)
EVERY = ("A", "B", "C", "B1")
CHUNK = 1 << 28  # bytes per device reduction / comparison: no 4-GiB temporary

#: name, batch, the frame id and the u64 offset of every row, dense (forms 3-4)
Table = namedtuple("Table", "name batch ids off dense")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Device:
    """The buffer, the placement that is written into it, and its tables."""

    def __init__(self, buf):
        self.buf = buf
        self.far, self.exp = fb.far(), fb.expect()
        self.current = None
        self._tables = self._recs = None

    def write(self, pl, frames):
        """Cluster by cluster, the bytes of `frames` (one per id, or a dict row -> frame over far.frames)."""
        K = self.far.K
        for c in range(3):
            if isinstance(frames, dict):
                rows = range(c * K, (c + 1) * K)
                data = np.frombuffer(b"".join(frames.get(r, self.far.frames[pl.ids[r]]) for r in rows), np.uint8)
            else:
                data = pl.cluster_bytes(frames, c)
            assert len(data) == pl.end[c] - pl.start[c]
            self.buf[pl.start[c]: pl.end[c]].copy_(_dev(data.copy()))

    def place(self, name):
        """Zero the old clusters, write the new ones; the buffer is never refilled."""
        pl = self.far.placements[name]
        if self.current != name:
            if self.current is not None:
                old = self.far.placements[self.current]
                for c in range(3):
                    self.buf[old.start[c]: old.end[c]].zero_()
            self.write(pl, self.far.frames)
            self.current, self._tables, self._recs = name, None, {}
        return pl

    def restore(self):
        self.write(self.far.placements[self.current], self.far.frames)

    def tables(self, name, forms=(1, 2, 3, 4), hints=True, views=True):
        """The placement's tables (built once per placement)."""
        pl = self.place(name)
        if self._tables is None:
            out = []
            o64, l32 = _dev(pl.off), _dev(pl.length.astype(np.int32))
            sizes = {"A": (BUFFER_BYTES, GIB4), "B": (BUFFER_BYTES, GIB4, NO_BASES_BYTES), "C": (BUFFER_BYTES, GIB4),
                     "B1": (NO_BASES_BYTES,)}[name]
            for size in sizes:
                n = pl.rows_within(size)
                vname = {BUFFER_BYTES: "whole", GIB4: "cut to 2^32", NO_BASES_BYTES: "cut to 2^32 - 1"}[size]
                for hint in ((0, abi.FRAMES_MONOTONE) if size == BUFFER_BYTES else (0,)):
                    b = FrameBatch(data=self.buf[:size], count=n, offsets=o64[:n], lengths=l32[:n], hints=hint)
                    tail = f"{vname}{' monotone' if hint else ''}"
                    out.append((1, hint, size, Table(f"form 1 {tail}", b, pl.ids[:n], pl.off[:n], False)))
                    out.append((2, hint, size, Table(f"form 2 {tail}", b.with_offsets32(), pl.ids[:n], pl.off[:n], False)))
            if name != "B1":
                b = FrameBatch(data=self.buf, count=len(pl.dense_ids), offsets=_dev(pl.dense_off))
                out.append((3, 0, BUFFER_BYTES, Table("form 3", b, pl.dense_ids, pl.dense_off[:-1], True)))
                out.append((4, 0, BUFFER_BYTES, Table("form 4", b.with_offsets32(), pl.dense_ids, pl.dense_off[:-1], True)))
            for form, _, size, t in out:  # the branch each table is there for
                bases = size > 0xFFFFFFFF and form in (2, 4)
                assert bool(t.batch.hints & abi.FRAMES_OFFSETS32) == (form in (2, 4))
                assert t.batch.offsets.numel() == (abi.offsets32_layout(t.batch.count, bases)[3] if form in (2, 4)
                                                   else t.batch.count + (form == 3))
            self._tables = out
        return [t for form, hint, size, t in self._tables
                if form in forms and (hints or not hint) and (views or size == BUFFER_BYTES)]

    def records(self, engine, t):
        """The device records of a table (parsed once per placement and table),
        checked against the oracle's: they are the second passes' input."""
        import torch
        if t.name not in self._recs:
            r = engine.parse(t.batch, VLAN, ParseMode.Strict, out_kind=abi.OUT_RECORD)
            torch.cuda.synchronize()
            helpers.records_equal(to_host(r, abi.RECORD_DTYPE, t.batch.count), self.exp.recs[t.ids], None,
                                  f"{self.current} {t.name}: records")
            self._recs[t.name] = r
        return self._recs[t.name]

    def others_are_zero(self, pl):
        """Every byte outside the clusters and their margins is zero (reductions on the device)."""
        edges = [0]
        for c in range(3):
            edges += [max(pl.start[c] - MARGIN, 0), pl.end[c] + MARGIN]
        edges.append(BUFFER_BYTES)
        for lo, hi in zip(edges[::2], edges[1::2]):
            for a in range(lo, hi, CHUNK):
                assert not bool(self.buf[a: min(a + CHUNK, hi)].any()), (pl.name, a)

    def clusters_equal(self, pl, want_frames, what):
        """The clusters' bytes with MARGIN bytes on each side equal `want_frames`
        (per id, or row -> frame) with zeros around them."""
        K = self.far.K
        for c in range(3):
            lo, hi = max(pl.start[c] - MARGIN, 0), pl.end[c] + MARGIN
            got = self.buf[lo:hi].cpu().numpy()
            want = np.zeros(hi - lo, np.uint8)
            if isinstance(want_frames, dict):
                rows = range(c * K, (c + 1) * K)
                body = np.frombuffer(b"".join(want_frames.get(r, self.far.frames[pl.ids[r]]) for r in rows), np.uint8)
            else:
                body = pl.cluster_bytes(want_frames, c)
            want[pl.start[c] - lo: pl.end[c] - lo] = body
            bad = np.nonzero(got != want)[0]
            if len(bad):
                p = lo + int(bad[0])
                r = int(np.searchsorted(pl.off, p, side="right")) - 1
                raise AssertionError(f"{what}: {len(bad)} bytes of cluster {c} differ; first at data byte {p:#x} (row {r}, "
                                     f"byte {p - int(pl.off[r])} of {int(pl.length[r])}): got {got[bad[0]]:#04x}, "
                                     f"want {want[bad[0]]:#04x}")


@pytest.fixture(scope="module")
def dev(engine, oracle):
    import torch
    torch.cuda.reset_peak_memory_stats()
    try:
        buf = torch.zeros(BUFFER_BYTES, dtype=torch.uint8, device="cuda")
    except RuntimeError as e:  # torch.OutOfMemoryError is one
        pytest.skip(f"a {BUFFER_BYTES}-B device allocation was refused: {e}")
    d = Device(buf)
    yield d
    del d.buf, buf
    torch.cuda.empty_cache()


# ---- raw entries into guarded outputs --------------------------------------------------------

def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def guarded(rows, row_bytes):
    import torch
    return torch.full(((rows + 2) * row_bytes,), SENTINEL, dtype=torch.uint8, device="cuda")


def unguard(t, rows, dtype, what):
    """The first `rows` rows on the host, after checking that the two spare rows kept their sentinel."""
    import torch
    torch.cuda.synchronize()
    h = t.cpu().numpy()
    nb = rows * np.dtype(dtype).itemsize
    assert len(h) == nb + 2 * np.dtype(dtype).itemsize and (h[nb:] == SENTINEL).all(), f"{what}: a store past out[count]"
    return h[:nb].view(dtype).copy()


def call(engine, fn, *args):
    rc = getattr(engine.lib, fn)(engine.ctx, *args, engine._stream(None))
    assert rc == abi.OK, (fn, engine.lib.nexg_ctx_last_error(engine.ctx))


def rows_equal(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype.names:
        bad = np.nonzero((got.view(np.uint8).reshape(len(got), -1) != want.view(np.uint8).reshape(len(want), -1)).any(axis=1))[0]
    else:
        bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (what, len(bad), int(bad[0]), got[bad[0]], want[bad[0]])


def parse_guarded(engine, t, kind, dtype, what):
    out = guarded(t.batch.count, dtype.itemsize)
    engine.parse(t.batch, VLAN, ParseMode.Strict, out_kind=kind, out=out)
    return unguard(out, t.batch.count, dtype, what)


# ---- the per-frame passes --------------------------------------------------------------------

def test_filler_rows(dev):
    """Each pass's expected row for a filler comes once from the 65535-byte
    zero frame and is the trivial row (tests/test_far_batch.py asserts the same
    of every pass on a machine without a GPU); the dense tables hold about
    65.6k of them."""
    exp, K = dev.exp, dev.far.K
    assert tuple(exp.match_filler)[:3] == (0, 0, abi.PAT_NONE)
    assert int(exp.recs["flags"][K]) == abi.L_ETHERNET and not exp.flows[K:].view(np.uint8).any()
    for pl in dev.far.placements.values():
        assert 65000 < pl.dense_is_filler.sum() < 66000


@pytest.mark.parametrize("name", EVERY)
def test_parse(engine, dev, name):
    """NEXG_OUT_RECORD and NEXG_OUT_DESC: the two-pass path for forms 1-2
    without the monotone hint, the span path with it and for forms 3-4."""
    exp = dev.exp
    for t in dev.tables(name):
        what = f"{name} {t.name}"
        helpers.records_equal(parse_guarded(engine, t, abi.OUT_RECORD, abi.RECORD_DTYPE, what), exp.recs[t.ids], None,
                              what + ": records")
        helpers.records_equal(parse_guarded(engine, t, abi.OUT_DESC, abi.DESC_DTYPE, what), exp.desc[t.ids], None,
                              what + ": descriptors")


@pytest.mark.parametrize("name", EVERY)
def test_checksum(engine, dev, name):
    exp = dev.exp
    for skip in (0xFFFFFFFF, 5):
        want = exp.checksum(skip)
        for t in dev.tables(name):
            fr = t.batch.to_c()
            out = guarded(t.batch.count, 2)
            call(engine, "nexg_checksum_batch", ctypes.byref(fr), skip, P(out))
            rows_equal(unguard(out, t.batch.count, np.dtype("<u2"), t.name), want[t.ids], f"{name} {t.name} skip {skip}")


@pytest.mark.parametrize("name", EVERY)
def test_decode_options(engine, dev, name):
    exp = dev.exp
    for t in dev.tables(name):
        fr = t.batch.to_c()
        out = guarded(t.batch.count, 96)
        call(engine, "nexg_decode_options", ctypes.byref(fr), P(dev.records(engine, t)), P(out))
        helpers.records_equal(unguard(out, t.batch.count, abi.OPTIONS_DTYPE, t.name), exp.options[t.ids], None,
                              f"{name} {t.name}: options")


def run_decap(engine, dev, t):
    """nexg_decap_batch into guarded outputs: (tunnels, inner_off, inner_len) device tensors and their host rows."""
    n = t.batch.count
    fr = t.batch.to_c()
    tun, off, ln = guarded(n, 16), guarded(n, 8), guarded(n, 4)
    opt = abi.DecapOption(abi.DECAP_VXLAN | abi.DECAP_GRE, abi.VXLAN_PORT, 0)
    call(engine, "nexg_decap_batch", ctypes.byref(fr), P(dev.records(engine, t)), ctypes.byref(opt), P(tun), P(off), P(ln))
    host = (unguard(tun, n, abi.TUNNEL_DTYPE, t.name), unguard(off, n, np.dtype("<u8"), t.name),
            unguard(ln, n, np.dtype("<u4"), t.name))
    return (tun, off, ln), host


def decap_want(exp, t):
    tun, rel, ln = exp.tunnels
    return tun[t.ids], (t.off + rel[t.ids]).astype(np.uint64), ln[t.ids]


@pytest.mark.parametrize("name", EVERY)
def test_decap(engine, dev, name):
    """Every inner_off is compared as a 64-bit value (the kernel stores it as two dwords)."""
    for t in dev.tables(name):
        _, (tun, off, ln) = run_decap(engine, dev, t)
        want_tun, want_off, want_ln = decap_want(dev.exp, t)
        helpers.records_equal(tun, want_tun, None, f"{name} {t.name}: tunnels")
        rows_equal(off, want_off, f"{name} {t.name}: inner_off")
        rows_equal(ln, want_ln, f"{name} {t.name}: inner_len")
        if name != "B1" and t.batch.data.numel() == BUFFER_BYTES:
            accepted = want_ln > 0
            assert (want_off[accepted] >= GIB4).sum() >= 10 and (want_off[accepted] < GIB4).sum() >= 10


@pytest.mark.parametrize("name", EVERY)
def test_dns(engine, dev, name):
    exp = dev.exp
    for t in dev.tables(name):
        n = t.batch.count
        want, tf_want, rows_want = exp.dns_rows(t.ids)
        total = len(rows_want)
        fr = t.batch.to_c()
        tiles = (n + 255) // 256
        out, tile_first, entries = guarded(n, 32), guarded(tiles + 1, 8), guarded(total, 16)
        opt = abi.DnsOption(0, abi.DNS_PORT, 0)
        call(engine, "nexg_dns_batch", ctypes.byref(fr), P(dev.records(engine, t)), ctypes.byref(opt), P(out), P(tile_first))
        call(engine, "nexg_dns_entries", ctypes.byref(fr), P(out), P(tile_first), P(entries), total)
        what = f"{name} {t.name}"
        helpers.records_equal(unguard(out, n, abi.DNS_DTYPE, what), want, None, what + ": summaries")
        rows_equal(unguard(tile_first, tiles + 1, np.dtype("<u8"), what), tf_want, what + ": tile_first")
        helpers.records_equal(unguard(entries, total, abi.DNS_ENTRY_DTYPE, what), rows_want, None, what + ": entries")


def run_match(engine, dev, t, frame_mode, records=True):
    n = t.batch.count
    fr = t.batch.to_c()
    pc = fb.pattern_set(frame_mode).to_c()
    out = guarded(n, 8)
    call(engine, "nexg_match_batch", ctypes.byref(fr), P(dev.records(engine, t)) if records else None, ctypes.byref(pc), P(out))
    return out, unguard(out, n, abi.MATCH_DTYPE, t.name)


@pytest.mark.parametrize("mode", (False, True), ids=("payload", "frame"))
@pytest.mark.parametrize("name", EVERY)
def test_match(engine, dev, name, mode):
    """Payload mode and frame mode (frame mode also without records)."""
    want = dev.exp.match(mode)
    for t in dev.tables(name):
        rows_equal(run_match(engine, dev, t, mode)[1], want[t.ids], f"{name} {t.name} frame={mode}")
        if mode:
            rows_equal(run_match(engine, dev, t, True, records=False)[1], want[t.ids], f"{name} {t.name} frame mode, NULL records")


def run_flow(engine, dev, t):
    n = t.batch.count
    fr = t.batch.to_c()
    fo = fb.FLOW_OPTION.to_c()
    out = guarded(n, 8)
    call(engine, "nexg_flow_batch", ctypes.byref(fr), P(dev.records(engine, t)), ctypes.byref(fo), P(out))
    return out, unguard(out, n, abi.FLOW_DTYPE, t.name)


@pytest.mark.parametrize("name", EVERY)
def test_flow(engine, dev, name):
    for t in dev.tables(name):
        rows_equal(run_flow(engine, dev, t)[1], dev.exp.flows[t.ids], f"{name} {t.name}: flow rows")


# ---- the in-place passes ---------------------------------------------------------------------

def per_row(pl, t, frames_out):
    """row of forms 1-2 -> the frame the pass leaves there, for the rows the table `t` holds."""
    if t.dense:
        return frames_out
    n = t.batch.count
    return {r: frames_out[pl.ids[r]] for r in range(n)}


@pytest.mark.parametrize("name", EVERY)
def test_recompute_checksums(engine, dev, name):
    exp = dev.exp
    frames_out, rows = exp.fixup
    for t in dev.tables(name):
        pl = dev.place(name)
        n = t.batch.count
        fr = t.batch.to_c()
        out = guarded(n, 8)
        opt = abi.ParseOptionC(FIX_OPTION.flags(ParseMode.Lenient), 0)
        call(engine, "nexg_recompute_checksums_batch", ctypes.byref(fr), ctypes.byref(opt), fb.BOTH, P(out))
        what = f"{name} {t.name}: fix-up"
        rows_equal(unguard(out, n, abi.FIXUP_DTYPE, what), rows[t.ids], what)
        dev.clusters_equal(pl, per_row(pl, t, frames_out), what)
        dev.others_are_zero(pl)
        dev.restore()
    dev.clusters_equal(pl, dev.far.frames, "restored")


@pytest.mark.parametrize("incremental", (False, True), ids=("recompute", "incremental"))
@pytest.mark.parametrize("name", EVERY)
def test_rewrite(engine, dev, name, incremental):
    """A 16-action set with an index (every action, and the values that mean none)."""
    frames_out, rows, index = dev.exp.rewrite(incremental)
    ac = fb.action_set(incremental).to_c()
    for t in dev.tables(name):
        pl = dev.place(name)
        n = t.batch.count
        fr = t.batch.to_c()
        out = guarded(n, 8)
        idx = _dev(index[t.ids])
        opt = abi.ParseOptionC(FIX_OPTION.flags(ParseMode.Lenient), 0)
        call(engine, "nexg_rewrite_batch", ctypes.byref(fr), ctypes.byref(opt), ctypes.byref(ac), P(idx), P(out))
        what = f"{name} {t.name}: rewrite incremental={incremental}"
        rows_equal(unguard(out, n, abi.REWRITTEN_DTYPE, what), rows[t.ids], what)
        dev.clusters_equal(pl, per_row(pl, t, frames_out), what)
        dev.others_are_zero(pl)
        dev.restore()
    dev.clusters_equal(pl, dev.far.frames, "restored")


# ---- the compactions -------------------------------------------------------------------------

def selection_outputs(count):
    import torch
    return (guarded(count, 4), guarded(count, 8), guarded(count, 4), torch.zeros(1, dtype=torch.int64, device="cuda"))


def check_selection(t, outs, pick, want_off, want_len, what):
    """out_index, out_off (64-bit) and out_len of a selection equal the picked rows of the table."""
    idx, off, ln, cnt = outs
    n = t.batch.count
    k = int(cnt.item())
    assert k == len(pick), (what, k, len(pick))
    hidx, hoff, hlen = (unguard(idx, n, np.dtype("<u4"), what), unguard(off, n, np.dtype("<u8"), what),
                        unguard(ln, n, np.dtype("<u4"), what))
    rows_equal(hidx[:k], pick.astype(np.uint32), what + ": out_index")
    rows_equal(hoff[:k], want_off[pick].astype(np.uint64), what + ": out_off")
    rows_equal(hlen[:k], want_len[pick].astype(np.uint32), what + ": out_len")
    return k


def run_select(engine, dev, t):
    """nexg_select_batch with FILTER and out_rule into guarded outputs: (outputs, rule tensor, workspace kept alive)."""
    n = t.batch.count
    fr = t.batch.to_c()
    fc = fb.FILTER.to_c()
    outs = selection_outputs(n)
    rule = guarded(n, 1)
    wsb = abi.select_workspace(n)
    ws = engine._workspace(wsb)
    call(engine, "nexg_select_batch", ctypes.byref(fr), P(dev.records(engine, t)), ctypes.byref(fc), P(outs[0]), P(outs[1]),
         P(outs[2]), P(rule), P(outs[3]), P(ws), wsb)
    return outs, rule


def table_lengths(dev, t):
    return dev.far.lengths[t.ids]


@pytest.mark.parametrize("name", EVERY)
def test_select(engine, dev, name):
    sel, rule_want = dev.exp.select
    for t in dev.tables(name, forms=(1, 2)):
        what = f"{name} {t.name}: select"
        outs, rule = run_select(engine, dev, t)
        pick = np.nonzero(sel[t.ids])[0]
        k = check_selection(t, outs, pick, t.off, table_lengths(dev, t), what)
        rows_equal(unguard(rule, t.batch.count, np.dtype("u1"), what)[:k], rule_want[t.ids][pick], what + ": out_rule")
        if t.batch.data.numel() == BUFFER_BYTES:
            assert (t.off[pick] >= GIB4).sum() >= 10 and len(set(rule_want[t.ids][pick].tolist())) >= 3


@pytest.mark.parametrize("name", EVERY)
def test_match_select(engine, dev, name):
    want_rows = dev.exp.match(False)
    for t in dev.tables(name, hints=False):
        what = f"{name} {t.name}: match_select"
        n = t.batch.count
        rows, _ = run_match(engine, dev, t, False)
        fr = t.batch.to_c()
        outs = selection_outputs(n)
        wsb = abi.match_select_workspace(n)
        ws = engine._workspace(wsb)
        call(engine, "nexg_match_select", ctypes.byref(fr), P(rows), fb.MATCH_ANY, 0, fb.MATCH_NONE, P(outs[0]), P(outs[1]),
             P(outs[2]), P(outs[3]), P(ws), wsb)
        pick = match_select_host(want_rows[t.ids], any=fb.MATCH_ANY, none=fb.MATCH_NONE).astype(np.int64)
        assert len(pick) >= 20
        check_selection(t, outs, pick, t.off, table_lengths(dev, t), what)


def inner_pick(exp, t, classes):
    tun = exp.tunnels[0][t.ids]
    return np.nonzero((tun["kind"] != abi.TUN_NONE) & (tun["status"] == abi.FRAME_OK) & np.isin(tun["inner"], list(classes)))[0]


def run_decap_select(engine, t, dec, classes):
    n = t.batch.count
    tun, off, ln = dec
    mask = 0
    for c in classes:
        mask |= 1 << int(c)
    outs = selection_outputs(n)
    wsb = abi.decap_select_workspace(n)
    ws = engine._workspace(wsb)
    call(engine, "nexg_decap_select", P(tun), P(off), P(ln), n, mask, P(outs[0]), P(outs[1]), P(outs[2]), P(outs[3]), P(ws), wsb)
    return outs


@pytest.mark.parametrize("name", EVERY)
def test_decap_select(engine, dev, name):
    for t in dev.tables(name, hints=False):
        dec, _ = run_decap(engine, dev, t)
        _, want_off, want_len = decap_want(dev.exp, t)
        for classes in ({abi.INNER_ETHERNET}, {abi.INNER_IPV4, abi.INNER_IPV6}):
            what = f"{name} {t.name}: decap_select {sorted(classes)}"
            pick = inner_pick(dev.exp, t, classes)
            assert len(pick) >= 10
            check_selection(t, run_decap_select(engine, t, dec, classes), pick, want_off, want_len, what)


# ---- chains over tables that hold offsets at and above 2^32 ----------------------------------

def selected_table(dev, t, outs):
    """The FrameBatch a selection's outputs describe (over the same data)."""
    import torch
    k = int(outs[3].item())
    return FrameBatch(data=t.batch.data, count=k, offsets=outs[1].view(torch.int64)[:k], lengths=outs[2].view(torch.int32)[:k],
                      hints=abi.FRAMES_MONOTONE)


@pytest.mark.parametrize("incremental", (False, True), ids=("recompute", "incremental"))
@pytest.mark.parametrize("name", fb.PLACEMENTS)
def test_select_then_rewrite_by_rule(engine, dev, name, incremental):
    """A match-action table: rule j of the filter gets action j, on the selected table."""
    sel, rule_want = dev.exp.select
    actions = fb.action_set(incremental)
    for t in dev.tables(name, forms=(1, 2), hints=False, views=False):
        pl = dev.place(name)
        outs, rule = run_select(engine, dev, t)
        tab = selected_table(dev, t, outs)
        rows = engine.rewrite(tab, actions, rule[: tab.count], FIX_OPTION)
        pick = np.nonzero(sel[t.ids])[0]
        assert tab.count == len(pick)
        frames = [dev.far.frames[i] for i in t.ids[pick]]
        want_frames, want_rows = rewrite_host(frames, actions, rule_want[t.ids][pick], FIX_OPTION)
        what = f"{name} {t.name}: select -> rewrite incremental={incremental}"
        rows_equal(to_host(rows, abi.REWRITTEN_DTYPE, tab.count), want_rows, what)
        assert ((want_rows["applied"] != 0) & (t.off[pick] >= GIB4)).sum() >= 10  # rewritten at and above 2^32
        dev.clusters_equal(pl, dict(zip(pick.tolist(), want_frames)), what)
        dev.others_are_zero(pl)
        dev.restore()


@pytest.mark.parametrize("name", fb.PLACEMENTS)
def test_decap_then_select_then_parse_of_the_inner_frames(engine, dev, name, oracle):
    exp = dev.exp
    for t in dev.tables(name, hints=False, views=False):
        dec, _ = run_decap(engine, dev, t)
        for classes, option, flags in (({abi.INNER_ETHERNET}, ParseOption(), 0),
                                       ({abi.INNER_IPV4, abi.INNER_IPV6}, FROM_IP, abi.PARSE_FROM_IP)):
            outs = run_decap_select(engine, t, dec, classes)
            tab = selected_table(dev, t, outs)
            pick = inner_pick(exp, t, classes)
            assert tab.count == len(pick)
            cut = []
            for i in t.ids[pick]:
                o, n = int(exp.tunnels[1][i]), int(exp.tunnels[2][i])
                cut.append(dev.far.frames[i][o: o + n])
            got = engine.parse_to_numpy(tab, option, out_kind=abi.OUT_RECORD)
            helpers.records_equal(got, oracle.parse_frames(cut, flags), cut, f"{name} {t.name}: inner parse {sorted(classes)}")


@pytest.mark.parametrize("name", fb.PLACEMENTS)
def test_select_then_gather_then_parse(engine, dev, name):
    exp = dev.exp
    sel, _ = exp.select
    for t in dev.tables(name, forms=(1, 2), hints=False, views=False):
        outs, _ = run_select(engine, dev, t)
        tab = selected_table(dev, t, outs)
        pick = np.nonzero(sel[t.ids])[0]
        ids = t.ids[pick]
        for align in (1, 16):
            what = f"{name} {t.name}: select -> gather align {align}"
            dense = engine.gather(tab, align)
            lens = dev.far.lengths[ids]
            slots = (lens + align - 1) // align * align
            want_off = np.concatenate([[0], np.cumsum(slots)]).astype(np.int64)
            assert dense.count == len(pick)
            rows_equal(to_host(dense.offsets, np.int64, len(pick) + 1), want_off, what + ": offsets")
            want = np.zeros(int(want_off[-1]), np.uint8)
            for o, i in zip(want_off[:-1], ids):
                want[o: o + len(dev.far.frames[i])] = np.frombuffer(dev.far.frames[i], np.uint8)
            assert dense.data.cpu().numpy()[: len(want)].tobytes() == want.tobytes(), what
            got = engine.parse_to_numpy(dense, VLAN, ParseMode.Strict, out_kind=abi.OUT_RECORD)
            helpers.records_equal(got, exp.recs[ids], None, what + ": parse")


# ---- the aggregates --------------------------------------------------------------------------

def host_batch(dev, t):
    """(frames, records, lengths, flow rows) of a table's rows, as the host contracts take them."""
    exp = dev.exp
    return [exp.frames[i] for i in t.ids], exp.recs[t.ids], exp.lengths[t.ids], exp.flows[t.ids]


@pytest.mark.parametrize("name", fb.PLACEMENTS)
def test_flow_partition_sort_and_groups(engine, dev, name):
    for t in dev.tables(name, forms=(1, 2), hints=False):
        what = f"{name} {t.name}"
        n = t.batch.count
        recs = dev.records(engine, t)
        flows, _ = run_flow(engine, dev, t)
        flows = flows[: n * 8]
        frames, hrecs, lengths, hflows = host_batch(dev, t)
        for buckets in (1, 7, 256):
            idx, table, first = engine.flow_partition(t.batch, flows, buckets)
            want_idx, want_first = partition_host(hflows["hash"], buckets)
            assert first.tolist() == want_first.tolist(), (what, buckets)
            rows_equal(to_host(idx, np.uint32, n), want_idx, f"{what}: partition index, {buckets} buckets")
            rows_equal(to_host(table.offsets, np.uint64, n), t.off[want_idx].astype(np.uint64), f"{what}: partition out_off")
            rows_equal(to_host(table.lengths, np.uint32, n), lengths[want_idx].astype(np.uint32), f"{what}: partition out_len")
        order = engine.flow_sort(flows)
        rows_equal(to_host(order, np.uint32, n), sort_host(hflows["hash"]), what + ": flow_sort")
        groups, group_of, k, _ = engine.flow_groups(t.batch, recs, flows, fb.FLOW_OPTION, order)
        want, want_of, want_k = groups_host(frames, hrecs, lengths, hflows, fb.FLOW_OPTION)
        assert k == want_k, (what, k, want_k)
        rows_equal(to_host(groups, abi.FLOW_GROUP_DTYPE, k), want, what + ": groups")
        rows_equal(to_host(group_of, np.uint32, n), want_of, what + ": group_of")
        assert (want["mixed"] > 0).sum() >= 1  # the collision pair: the key compare read both frames' bytes


@pytest.mark.parametrize("form", (1, 2))
def test_flow_table_over_the_placements_as_epochs(engine, dev, form):
    """FlowTable.update over A, B, C as epochs 0, 1, 2 (grown from capacity 1),
    against merge_host and the dictionary of tests/flow_table_ref.py."""
    exp = dev.exp
    table = FlowTable(engine, fb.FLOW_OPTION, capacity=1)
    host = np.zeros(0, abi.FLOW_ENTRY_DTYPE)
    refd = tr.RefTable(False, True)
    for epoch, name in enumerate(fb.PLACEMENTS):
        t, = dev.tables(name, forms=(form,), hints=False, views=False)
        frames, recs, lengths, flows = host_batch(dev, t)
        groups, group_of, _ = groups_host(frames, recs, lengths, flows, fb.FLOW_OPTION)
        host, want_slot = merge_host(host, groups, frames, recs, lengths, fb.FLOW_OPTION, epoch, 0)
        refd.feed(frames, recs, lengths, flows["hash"], epoch, 0)
        slot, gof = table.update(t.batch, dev.records(engine, t), epoch)
        got = table.rows()
        tr.entries_equal(got, host, (name, t.name, "merge_host"))
        tr.entries_equal(got, refd.rows(), (name, t.name, "reference"))
        row = to_host(slot, np.uint32, slot.numel())[to_host(gof, np.uint32, t.batch.count)]
        assert (row == want_slot[group_of]).all(), (name, t.name)
    assert int(got["packets"].sum()) == 9 * dev.far.K and int(got["flags8"].sum()) >= 1


# ---- gather past 4 GiB -----------------------------------------------------------------------

def test_gather_of_the_dense_table_past_4_gib(engine, dev):
    """nexg_gather_plan + nexg_gather_frames with align 1 over the whole of
    form 3 into a second buffer: the plan's 64-bit scan and the copy's chunk
    index both cross 2^32, and the output is data[1 : 1 + total]."""
    import torch
    t, = dev.tables("A", forms=(3,))
    pl = dev.place("A")
    n = t.batch.count
    total = int(pl.dense_off[-1] - pl.dense_off[0])
    assert total > GIB4 and (n + 255) // 256 > 256
    fr = t.batch.to_c()
    offs = guarded(n + 1, 8)
    wsb = abi.gather_plan_workspace(n)
    ws = engine._workspace(wsb)
    call(engine, "nexg_gather_plan", ctypes.byref(fr), 1, P(offs), None, P(ws), wsb)
    hoffs = unguard(offs, n + 1, np.dtype("<u8"), "gather_plan")
    rows_equal(hoffs, (pl.dense_off - 1).astype(np.uint64), "gather_plan: out_offsets")
    assert int(hoffs[n]) == total
    try:
        out = torch.empty(total + 4096, dtype=torch.uint8, device="cuda")
    except RuntimeError as e:  # torch.OutOfMemoryError is one
        pytest.skip(f"a second {total}-B device allocation was refused: {e}")
    out[total:].fill_(SENTINEL)
    call(engine, "nexg_gather_frames", ctypes.byref(fr), P(offs), P(out), total)
    torch.cuda.synchronize()
    for a in range(0, total, CHUNK):
        b = min(a + CHUNK, total)
        assert torch.equal(out[a:b], dev.buf[1 + a: 1 + b]), f"gather_frames: bytes {a:#x}..{b:#x}"
    assert bool((out[total:] == SENTINEL).all()), "a store past out[total]"
    del out
    torch.cuda.empty_cache()


def test_peak_device_memory(dev):
    """The buffer, the second buffer of the gather test and the small rest: under 10 GiB."""
    import torch
    peak = torch.cuda.max_memory_allocated()
    print(f"far batch: peak device memory {peak / 2**30:.2f} GiB")
    assert BUFFER_BYTES <= peak < 10 << 30, peak
