"""GPU: flow rows (nexg_flow_batch) and the flow-affine partition
(nexg_flow_partition) on the corpus of tests/flow_frames.py.

The expectation is nex_amd.flow.flow_host / partition_host (pinned by the
published RSS vectors and the truth table in tests/test_flow_host.py) applied
to the oracle's records of the corpus, computed once per option and tiled to
each count. Shapes: the counts around a wave, a 256-frame block, the
partition's 1024-frame tile and its scan (65793 frames = 65 tiles; 262145 =
257 tiles; 1048577 frames at 256 buckets = 257 chunks of 1024 counters, so
the one-workgroup scan of the chunk sums carries into a second step); the
layouts tests/test_gpu_select.py uses; records that point past their frame;
the passes composed with parse, decap, gather_rows and gather."""
import ctypes
import itertools

import numpy as np
import pytest

from nex_amd import abi
from nex_amd.engine import FrameBatch
from nex_amd.flow import FlowOption, flows_host, partition_host
from nex_amd.frame import ParseMode, ParseOption
from tests import flow_frames as ff
from tests import helpers
from tests.helpers import layouts, parse_records, to_host
from tests.test_gpu_select import table_of

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1000, 65793]
PART_COUNTS = [0, 1, 255, 256, 257, 1023, 1024, 1025, 65793]
BUCKETS = (1, 2, 3, 8, 255, 256)
VLAN = ParseOption(unwrap_vlan=True)
OTHER_KEY = bytes((37 * i + 11) & 0xFF for i in range(40))
#: every option combination (run on the first layout); the first two run on every layout
OPTIONS = [(f"sym={s} ports={p} key={'custom' if k else 'default'}", FlowOption(symmetric=s, ports=p, key=k))
           for k, p, s in itertools.product((None, OTHER_KEY), (True, False), (False, True))]
assert OPTIONS[0][1] == FlowOption() and OPTIONS[1][1] == FlowOption(symmetric=True)


class Corpus:
    """The corpus, the oracle's records, and flow_host's rows per option
    (computed once per option, cached by name)."""

    def __init__(self, oracle):
        self.items = ff.corpus()
        self.frames = [x.frame for x in self.items]
        self.recs = oracle.parse_frames(self.frames, ff.PARSE_FLAGS)
        self.cache = {}

    def rows(self, name, option):
        if name not in self.cache:
            self.cache[name] = flows_host(self.frames, self.recs, [len(f) for f in self.frames], option)
        return self.cache[name]

    def tiled(self, count):
        which = np.arange(count) % len(self.frames)
        return which, [self.frames[i] for i in which]


@pytest.fixture(scope="module")
def corp(oracle):
    return Corpus(oracle)


def flows_equal(got, want, name):
    for n in abi.FLOW_DTYPE.names:
        bad = np.nonzero(got[n] != want[n])[0]
        assert len(bad) == 0, (name, n, int(bad[0]), int(got[n][bad[0]]), int(want[n][bad[0]]))


# ---- Engine.flow ------------------------------------------------------------------------

@pytest.mark.parametrize("count", COUNTS)
def test_flow_parity_every_layout(engine, corp, count):
    which, frames = corp.tiled(count)
    for li, (lname, batch, keep) in enumerate(layouts(frames, only_first=count > 1000)):
        w = which if keep is None else which[keep]
        recs = parse_records(engine, batch)
        if count == 1000 and li == 0:  # the device records are the oracle's (the expectation's input)
            helpers.records_equal(to_host(recs, abi.RECORD_DTYPE, count), corp.recs[which], frames, "records")
        for oname, opt in (OPTIONS if li == 0 else OPTIONS[:2]):
            got = to_host(engine.flow(batch, recs, opt), abi.FLOW_DTYPE, batch.count)
            flows_equal(got, corp.rows(oname, opt)[w], f"{lname} n={count} {oname}")


def test_golden_hashes_come_back_from_the_device(engine, corp):
    batch = FrameBatch.from_packed(corp.frames, pad_to=1)
    recs = parse_records(engine, batch)
    l4 = to_host(engine.flow(batch, recs), abi.FLOW_DTYPE, batch.count)
    ipo = to_host(engine.flow(batch, recs, FlowOption(ports=False)), abi.FLOW_DTYPE, batch.count)
    n = 0
    for i, x in enumerate(corp.items):
        if x.hash_l4 is not None:
            assert int(l4["hash"][i]) == x.hash_l4 and int(ipo["hash"][i]) == x.hash_ip, x.what
            n += 1
        if x.kind is not None:
            assert int(l4["kind"][i]) == x.kind and int(l4["proto"][i]) == (x.proto if x.kind else 0), x.what
    assert n == 16


def test_hostile_records(engine, corp):
    """Records are caller memory: l3_off at, just past and far past the frame,
    an IPv6 header that ends one byte around the frame's end, a claimed IPv6
    layer on a frame that has none, payload_off + payload_len past the frame,
    and an IPv6 header that ends on the data tensor's last byte. Nothing
    faults, the row is flow_host's on the same records, and every IPv6 record
    whose l3_off + 40 leaves its frame gives the all-zero row."""
    import torch
    base = [f for f in corp.frames if len(f) < 2000]
    v6 = next(x.frame for x in corp.items if x.what == "vector 5 udp")
    frames = (base * 5)[:299] + [v6]  # the last frame ends on the data tensor's last byte
    batch = FrameBatch.from_packed(frames, pad_to=1)
    assert batch.data.numel() == sum(len(f) for f in frames)
    recs = parse_records(engine, batch)
    torch.cuda.synchronize()
    h = to_host(recs, abi.RECORD_DTYPE, len(frames))
    rng = np.random.default_rng(5)
    for i in range(len(frames)):
        k = i % 7
        if k == 1:
            h["l3_off"][i] = len(frames[i]) + int(rng.integers(0, 3))
        elif k == 2:
            h["l3_off"][i] = 65535
        elif k == 3:
            h["l3_off"][i] = max(0, len(frames[i]) - 40 + int(rng.integers(-1, 2)))
        elif k == 4:
            h["flags"][i] = (int(h["flags"][i]) | abi.L_IPV6) & ~abi.L_IPV4
        elif k == 5:
            h["payload_off"][i] = len(frames[i]) - 1
            h["payload_len"][i] = 65535
    last = len(frames) - 1
    h["l3_off"][last] = len(v6) - 40  # ends exactly on the last byte of the data
    h["flags"][last] = abi.L_ETHERNET | abi.L_IP | abi.L_IPV6
    dev = torch.from_numpy(h.view(np.uint8).copy()).cuda()
    for oname, opt in OPTIONS[:2]:
        want = flows_host(frames, h, [len(f) for f in frames], opt)
        got = to_host(engine.flow(batch, dev, opt), abi.FLOW_DTYPE, len(frames))
        flows_equal(got, want, f"hostile {oname}")
        v6rec = ((h["flags"] & abi.L_IPV6) != 0) & ((h["flags"] & abi.L_IPV4) == 0)
        out = v6rec & (h["l3_off"].astype(np.int64) + 40 > np.array([len(f) for f in frames]))
        assert out.sum() > 20 and not got.view(np.uint64)[out].any()
        assert int(got["kind"][last]) == abi.FLOW_IPV6 and int(got["hash"][last]) != 0  # read from the very end of the data


def test_flow_on_a_decap_inner_table(engine, oracle):
    """The pass works unchanged on an inner table with the inner records."""
    from tests import tunnel_frames as tf
    cs = tf.cycled(tf.cases(), 300)
    batch = FrameBatch.from_packed([c.frame for c in cs], pad_to=1)
    recs = engine.parse(batch, VLAN, out_kind=abi.OUT_RECORD)
    tunnels, inner = engine.decap(batch, recs)
    oidx, eth = engine.decap_select(tunnels, inner, {abi.INNER_ETHERNET})
    rec_eth = engine.parse(eth, out_kind=abi.OUT_RECORD)
    wrapped = [cs[i].inner for i in to_host(oidx, np.uint32, eth.count)]
    assert len(wrapped) > 50 and all(w is not None for w in wrapped)
    want_recs = oracle.parse_frames(wrapped)
    for opt in (FlowOption(), FlowOption(symmetric=True)):
        want = flows_host(wrapped, want_recs, [len(f) for f in wrapped], opt)
        assert (want["kind"] != 0).sum() > 20
        flows_equal(to_host(engine.flow(eth, rec_eth, opt), abi.FLOW_DTYPE, eth.count), want, "inner")


def test_flow_rejections(engine, corp):
    import torch
    batch = FrameBatch.from_packed(corp.frames, pad_to=1)
    recs = parse_records(engine, batch)
    out = torch.zeros(batch.count * 8 + 8, dtype=torch.uint8, device="cuda")
    fr = batch.to_c()
    P = ctypes.c_void_p

    def call(opt, r=recs.data_ptr(), o=out.data_ptr()):
        return engine.lib.nexg_flow_batch(engine.ctx, ctypes.byref(fr), P(r) if r else None,
                                          None if opt is None else ctypes.byref(opt), P(o) if o else None,
                                          engine._stream(None))

    assert call(None) == abi.OK  # NULL option = defaults
    torch.cuda.synchronize()
    flows_equal(to_host(out, abi.FLOW_DTYPE, batch.count), corp.rows(*OPTIONS[0]), "NULL option")
    assert call(FlowOption(flags=0x8).to_c(validate=False)) == abi.EINVAL
    assert call(FlowOption(reserved=1).to_c(validate=False)) == abi.EINVAL
    assert call(None, r=0) == abi.EINVAL and call(None, o=0) == abi.EINVAL
    assert call(None, o=out.data_ptr() + 4) == abi.EINVAL and call(None, r=recs.data_ptr() + 8) == abi.EINVAL
    with pytest.raises(ValueError):
        engine.flow(batch, recs, FlowOption(flags=0x10))
    empty = FrameBatch.from_packed([], pad_to=1)
    ef = empty.to_c()
    assert engine.lib.nexg_flow_batch(engine.ctx, ctypes.byref(ef), None, None, None, engine._stream(None)) == abi.OK


# ---- Engine.flow_partition ----------------------------------------------------------------

def dummy_batch(count):
    """`count` 4-byte frames at a fixed stride: the partition reads no frame byte."""
    import torch
    return FrameBatch(data=torch.zeros(max(count, 4) * 4, dtype=torch.uint8, device="cuda"), count=count, stride=4)


def flows_from_hashes(hashes):
    import torch
    rows = np.zeros(len(hashes), abi.FLOW_DTYPE)
    rows["hash"] = hashes
    rows["kind"] = abi.FLOW_IPV4
    return torch.from_numpy(rows.view(np.uint8).copy()).cuda()


def check_partition(engine, name, batch, flows, hashes, buckets):
    idx, table, first = engine.flow_partition(batch, flows, buckets)
    want_idx, want_first = partition_host(hashes, buckets)
    assert first.dtype == np.int64 and first.tolist() == want_first.tolist(), name
    got = to_host(idx, np.uint32, batch.count)
    bad = np.nonzero(got != want_idx)[0]
    assert len(bad) == 0, (name, int(bad[0]), int(got[bad[0]]), int(want_idx[bad[0]]))
    off, ln = table_of(batch)
    assert table.count == batch.count and table.data.data_ptr() == batch.data.data_ptr()
    assert (to_host(table.offsets, np.int64, batch.count) == off[want_idx]).all(), name
    assert (to_host(table.lengths, np.uint32, batch.count) == ln[want_idx]).all(), name
    return idx, table, first


@pytest.mark.parametrize("count", PART_COUNTS)
def test_partition_parity(engine, corp, count):
    which, frames = corp.tiled(count)
    want = corp.rows(*OPTIONS[0])[which]
    for lname, batch, keep in layouts(frames, only_first=count > 1025):
        recs = parse_records(engine, batch)
        flows = engine.flow(batch, recs)
        hashes = want["hash"] if keep is None else want["hash"][keep]
        for buckets in BUCKETS:
            check_partition(engine, f"{lname} n={count} buckets={buckets}", batch, flows, hashes, buckets)


@pytest.mark.parametrize("count", [262145, 1048577])
def test_partition_large_counts_arbitrary_hashes(engine, count):
    """More than 256 tiles, and (at 256 buckets) more than 256 chunks of
    counters: both levels of the scan carry. The hashes are the test's own."""
    rng = np.random.default_rng(count)
    hashes = rng.integers(0, 1 << 32, count, dtype=np.uint64).astype(np.uint32)
    hashes[:: 13] = 0xFFFFFFFF
    hashes[5:: 17] = 0
    batch, flows = dummy_batch(count), flows_from_hashes(hashes)
    for buckets in BUCKETS:
        check_partition(engine, f"n={count} buckets={buckets}", batch, flows, hashes, buckets)


def test_partition_is_deterministic(engine, corp):
    import torch
    which, frames = corp.tiled(65793)
    batch = FrameBatch.from_packed(frames, pad_to=1)
    flows = engine.flow(batch, parse_records(engine, batch))
    for buckets in (8, 256):
        runs = []
        for _ in range(2):
            idx, table, first = engine.flow_partition(batch, flows, buckets)
            runs.append((idx.clone(), table.offsets.clone(), table.lengths.clone(), torch.from_numpy(first)))
        for a, b in zip(*runs):
            assert torch.equal(a, b), buckets


def test_partition_one_bucket_and_all_buckets(engine):
    n = 3000
    batch = dummy_batch(n)
    same = np.full(n, 0x51CCC17D, np.uint32)  # % 8 == 5
    idx, table, first = check_partition(engine, "one bucket", batch, flows_from_hashes(same), same, 8)
    assert first.tolist() == [0] * 6 + [n] * 3 and (to_host(idx, np.uint32, n) == np.arange(n)).all()
    every = (np.arange(n, dtype=np.uint32) * 2654435761 % 256).astype(np.uint32) + 256 * np.arange(n, dtype=np.uint32)
    idx, table, first = check_partition(engine, "all buckets", batch, flows_from_hashes(every), every, 256)
    assert (np.diff(first) > 0).all()


def _raw_partition(engine, batch, flows, buckets, idx, off, ln, first, ws, ws_bytes):
    fr = batch.to_c()
    p = lambda t: None if t is None else ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())  # noqa: E731
    return engine.lib.nexg_flow_partition(engine.ctx, ctypes.byref(fr), p(flows), buckets, p(idx), p(off), p(ln),
                                          p(first), p(ws), ws_bytes, engine._stream(None))


def test_partition_stores_stay_inside_the_outputs(engine):
    """flows and the workspace are caller memory: with arbitrary rows (every
    byte random) and a workspace full of ones beforehand, the result is the
    stable partition of those hashes and nothing is stored past `count`
    entries or past bucket_first's buckets + 1."""
    import torch
    n, buckets, guard = 5000, 37, 64
    rng = np.random.default_rng(11)
    raw = rng.integers(0, 256, n * 8, dtype=np.uint8)
    hashes = raw.view(abi.FLOW_DTYPE)["hash"].copy()
    flows = torch.from_numpy(raw).cuda()
    batch = dummy_batch(n)
    idx = torch.full((n + guard,), -7, dtype=torch.int32, device="cuda")
    off = torch.full((n + guard,), -7, dtype=torch.int64, device="cuda")
    ln = torch.full((n + guard,), -7, dtype=torch.int32, device="cuda")
    first = torch.full((buckets + 1 + guard,), -7, dtype=torch.int64, device="cuda")
    wsb = abi.flow_partition_workspace(n, buckets)
    ws = torch.full(((wsb + 7) // 8 + guard,), -1, dtype=torch.int64, device="cuda")
    assert _raw_partition(engine, batch, flows, buckets, idx, off, ln, first, ws, wsb) == abi.OK
    torch.cuda.synchronize()
    want_idx, want_first = partition_host(hashes, buckets)
    assert (to_host(idx, np.uint32, n) == want_idx).all()
    assert first[: buckets + 1].cpu().numpy().tolist() == want_first.tolist()
    assert (to_host(off, np.int64, n) == want_idx.astype(np.int64) * 4).all() and (to_host(ln, np.uint32, n) == 4).all()
    for t in (idx[n:], off[n:], ln[n:], first[buckets + 1:]):
        assert bool((t == -7).all())
    assert bool((ws[(wsb + 7) // 8:] == -1).all())
    # out_off / out_len may both be NULL
    idx.fill_(-7)
    assert _raw_partition(engine, batch, flows, buckets, idx, None, None, first, ws, wsb) == abi.OK
    torch.cuda.synchronize()
    assert (to_host(idx, np.uint32, n) == want_idx).all()


def test_partition_rejections(engine):
    import torch
    n, buckets = 3000, 8
    batch = dummy_batch(n)
    flows = flows_from_hashes(np.arange(n, dtype=np.uint32))
    idx = torch.zeros(n + 4, dtype=torch.int32, device="cuda")
    off = torch.zeros(n + 4, dtype=torch.int64, device="cuda")
    ln = torch.zeros(n + 4, dtype=torch.int32, device="cuda")
    first = torch.zeros(260, dtype=torch.int64, device="cuda")
    wsb = abi.flow_partition_workspace(n, buckets)
    ws = torch.zeros(wsb // 8 + 2, dtype=torch.int64, device="cuda")
    good = dict(flows=flows, buckets=buckets, idx=idx, off=off, ln=ln, first=first, ws=ws, ws_bytes=wsb)
    assert _raw_partition(engine, batch, **good) == abi.OK
    assert _raw_partition(engine, batch, **dict(good, ws_bytes=wsb - 1)) == abi.EINVAL
    assert b"workspace" in engine.lib.nexg_ctx_last_error(engine.ctx)
    for bad in (0, 257, 1 << 16):
        assert _raw_partition(engine, batch, **dict(good, buckets=bad)) == abi.EINVAL, bad
    for key in ("flows", "idx", "first", "ws", "off", "ln"):  # off or ln alone NULL: they go together
        assert _raw_partition(engine, batch, **dict(good, **{key: None})) == abi.EINVAL, key
    for key, t, step in (("flows", flows, 4), ("idx", idx, 2), ("off", off, 4), ("ln", ln, 2), ("first", first, 4),
                         ("ws", ws, 4)):
        assert _raw_partition(engine, batch, **dict(good, **{key: t.data_ptr() + step})) == abi.EINVAL, key
    with pytest.raises(ValueError):
        engine.flow_partition(batch, flows, 257)
    # count == 0 writes bucket_first[0..buckets] = 0 and needs nothing else
    first.fill_(7)
    assert _raw_partition(engine, dummy_batch(0), None, buckets, None, None, None, first, None, 0) == abi.OK
    torch.cuda.synchronize()
    assert first[: buckets + 2].cpu().numpy().tolist() == [0] * (buckets + 1) + [7]


# ---- composition ---------------------------------------------------------------------------

def test_parse_and_gather_of_each_bucket(engine, corp):
    """Parsing bucket b's table gives gather_rows(records, 64, index[first:last]);
    Engine.gather of a bucket gives a dense batch that parses to the same records."""
    which, frames = corp.tiled(700)
    batch = FrameBatch.from_packed(frames, pad_to=1)
    recs = parse_records(engine, batch)
    flows = engine.flow(batch, recs)
    buckets = 8
    idx, table, first = engine.flow_partition(batch, flows, buckets)
    want_idx, _ = partition_host(corp.rows(*OPTIONS[0])["hash"][which], buckets)
    hidx = to_host(idx, np.uint32, batch.count)
    assert (hidx == want_idx).all()
    by_bucket = engine.gather_rows(recs, 64, idx)
    for b in range(buckets):
        lo, hi = int(first[b]), int(first[b + 1])
        part = engine.flow_bucket(table, first, b)
        assert part.count == hi - lo > 0 and part.data.data_ptr() == batch.data.data_ptr()
        assert part.offsets.data_ptr() == table.offsets.data_ptr() + 8 * lo  # a view: nothing is copied
        got = engine.parse_to_numpy(part, VLAN, ParseMode.Strict, out_kind=abi.OUT_RECORD)
        rows = to_host(engine.gather_rows(recs, 64, idx[lo:hi]), abi.RECORD_DTYPE, hi - lo)
        pick = hidx[lo:hi]
        helpers.records_equal(got, rows, [frames[i] for i in pick], f"parse(bucket {b})")
        helpers.records_equal(rows, corp.recs[which][pick], None, f"gather_rows(bucket {b})")
        assert rows.tobytes() == to_host(by_bucket, abi.RECORD_DTYPE, batch.count)[lo:hi].tobytes()
        if b in (0, 5):
            dense = engine.gather(part)
            assert dense.data.data_ptr() != batch.data.data_ptr()
            got = engine.parse_to_numpy(dense, VLAN, ParseMode.Strict, out_kind=abi.OUT_RECORD)
            helpers.records_equal(got, rows, [frames[i] for i in pick], f"parse(gather(bucket {b}))")


def test_symmetric_conversations_share_a_bucket(engine, corp):
    batch = FrameBatch.from_packed(corp.frames, pad_to=1)
    recs = parse_records(engine, batch)
    flows = engine.flow(batch, recs, FlowOption(symmetric=True))
    idx, table, first = engine.flow_partition(batch, flows, 8)
    hidx = to_host(idx, np.uint32, batch.count)
    bucket_of = np.zeros(batch.count, np.int64)
    for b in range(8):
        bucket_of[hidx[int(first[b]): int(first[b + 1])]] = b
    convs = {}
    for i, x in enumerate(corp.items):
        if x.conv:
            convs.setdefault(x.conv, set()).add(int(bucket_of[i]))
    assert len(convs) >= 18 and all(len(s) == 1 for s in convs.values()), convs
    assert len({next(iter(s)) for s in convs.values()}) > 2  # and they do spread over the buckets
