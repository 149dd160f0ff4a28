"""GPU: the sort of a batch by flow hash (nexg_flow_sort) and its reduction to
one row per flow (nexg_flow_groups).

The expectation is nex_amd.flow.sort_host / groups_host (checked against an
independent group-by in tests/test_flow_groups_host.py) on the oracle's records
of the corpus of tests/flow_frames.py plus the pinned collision pair, tiled to
each count; for the fabricated batches (one flow, singletons, runs that cross
tile borders) the expectation is numpy on the test's own construction. Shapes:
the counts around a wave, a 256-position tile, the sort's 1024-frame tile and
its counter scan (65793 frames = 65 sort tiles and 258 group tiles; 1048577
frames = 257 chunks of 1024 counters per digit pass, so both levels of the
scan carry); every layout of tests.helpers.layouts; caller memory that
holds anything."""
import ctypes
import subprocess

import numpy as np
import pytest

from nex_amd import abi
from nex_amd.engine import FrameBatch
from nex_amd.flow import FlowOption, flows_host, groups_host, sort_host
from tests import flow_frames as ff
from tests import flow_group_frames as fg
from tests.helpers import build_native_test, layouts, parse_records, to_host
from tests.test_gpu_flow import flows_from_hashes

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 65793]
OPTIONS = [(f"sym={s} ports={p}", FlowOption(symmetric=s, ports=p)) for s in (False, True) for p in (True, False)]
GROUP_FIELDS = abi.FLOW_GROUP_DTYPE.names


class Corpus:
    """The corpus with the collision pair, the oracle's records, flow_host's
    rows and each frame's key per option (computed once per option)."""

    def __init__(self, oracle):
        self.frames = [x.frame for x in ff.corpus()] + fg.collision_frames()
        self.recs = oracle.parse_frames(self.frames, ff.PARSE_FLAGS)
        self.lengths = np.array([len(f) for f in self.frames])
        self.cache = {}

    def rows(self, name, option):
        if name not in self.cache:
            self.cache[name] = flows_host(self.frames, self.recs, self.lengths, option)
        return self.cache[name]

    def tiled(self, count):
        which = np.arange(count) % len(self.frames)
        return which, [self.frames[i] for i in which]

    def groups(self, w, name, option, order=None, flows=None):
        """groups_host of the frames `w` names (corpus indices, in batch order)."""
        flows = self.rows(name, option)[w] if flows is None else flows
        return groups_host([self.frames[i] for i in w], self.recs[w], self.lengths[w], flows, option, order)


@pytest.fixture(scope="module")
def corp(oracle):
    return Corpus(oracle)


def groups_equal(got, want, name):
    assert len(got) == len(want), (name, len(got), len(want))
    for n in GROUP_FIELDS:
        bad = np.nonzero(got[n] != want[n])[0]
        assert len(bad) == 0, (name, n, int(bad[0]), got[bad[0]], want[bad[0]])


def run_groups(engine, batch, recs, flows, option=None, order=None):
    """Engine.flow_groups' result on the host: (groups, group_of, n, order)."""
    groups, group_of, n, order = engine.flow_groups(batch, recs, flows, option, order)
    return (to_host(groups, abi.FLOW_GROUP_DTYPE, n), to_host(group_of, np.uint32, batch.count), n,
            to_host(order, np.uint32, batch.count))


# ---- Engine.flow_sort ------------------------------------------------------------------------

def check_sort(engine, name, hashes, flows=None):
    flows = flows_from_hashes(hashes) if flows is None else flows
    got = to_host(engine.flow_sort(flows), np.uint32, len(hashes))
    want = sort_host(hashes)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (name, int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))


@pytest.mark.parametrize("count", COUNTS)
def test_sort_parity_on_the_corpus(engine, corp, count):
    which, frames = corp.tiled(count)
    batch = FrameBatch.from_packed(frames, pad_to=1)
    for oname, opt in OPTIONS[:2]:
        flows = engine.flow(batch, parse_records(engine, batch), opt)
        check_sort(engine, f"n={count} {oname}", corp.rows(oname, opt)["hash"][which], flows)


@pytest.mark.parametrize("count", [262145, 1048577])
def test_sort_large_counts_arbitrary_hashes(engine, count):
    """More than 256 sort tiles, and at 1048577 more than 256 chunks of
    counters in every digit pass: both levels of the scan carry. Runs of
    0xFFFFFFFF and of 0, and all 256 values of the top byte."""
    rng = np.random.default_rng(count)
    hashes = rng.integers(0, 1 << 32, count, dtype=np.uint64).astype(np.uint32)
    hashes[:: 13] = 0xFFFFFFFF
    hashes[5:: 17] = 0
    hashes[1000: 3000] = 0xFFFFFFFF
    hashes[7000: 9000] = 0
    assert len(np.unique(hashes >> 24)) == 256
    check_sort(engine, f"n={count}", hashes)


def test_sort_of_equal_hashes_is_the_identity(engine):
    for n in (1, 1025, 70000):
        for h in (0, 0x51CCC17D, 0xFFFFFFFF):
            hashes = np.full(n, h, np.uint32)
            got = to_host(engine.flow_sort(flows_from_hashes(hashes)), np.uint32, n)
            assert (got == np.arange(n)).all(), (n, h)


@pytest.mark.parametrize("byte", [0, 1, 2, 3])
def test_sort_each_digit_pass_alone(engine, byte):
    """Hashes that differ in one byte only: that pass must order them, and the
    other three must keep what it did (or will find) intact."""
    n = 5000
    rng = np.random.default_rng(byte)
    digit = rng.integers(0, 256, n, dtype=np.uint64).astype(np.uint32)
    fixed = 0xA5C33C5A & ~(0xFF << (8 * byte)) & 0xFFFFFFFF
    hashes = (np.uint32(fixed) | (digit << np.uint32(8 * byte))).astype(np.uint32)
    assert len(np.unique(hashes)) == 256
    check_sort(engine, f"byte {byte}", hashes)


def test_sort_is_deterministic_and_ignores_the_workspace(engine, corp):
    """Two runs at 65793 give the same bytes; so does a raw call whose
    workspace was full of ones beforehand, with nothing stored past `count`
    entries or past the workspace."""
    import torch
    which, frames = corp.tiled(65793)
    batch = FrameBatch.from_packed(frames, pad_to=1)
    flows = engine.flow(batch, parse_records(engine, batch))
    a, b = engine.flow_sort(flows).clone(), engine.flow_sort(flows).clone()
    assert torch.equal(a, b)
    n, guard = batch.count, 64
    wsb = abi.flow_sort_workspace(n)
    ws = torch.full((wsb // 8 + guard,), -1, dtype=torch.int64, device="cuda")
    idx = torch.full((n + guard,), -7, dtype=torch.int32, device="cuda")
    assert _raw_sort(engine, flows, n, idx, ws, wsb) == abi.OK
    torch.cuda.synchronize()
    assert torch.equal(idx[:n], a) and bool((idx[n:] == -7).all()) and bool((ws[wsb // 8:] == -1).all())
    assert (to_host(a, np.uint32, n) == sort_host(corp.rows(*OPTIONS[0])["hash"][which])).all()


def test_sort_of_arbitrary_flow_bytes(engine):
    """flows is caller memory: every byte random."""
    import torch
    n = 5000
    raw = np.random.default_rng(12).integers(0, 256, n * 8, dtype=np.uint8)
    check_sort(engine, "random rows", raw.view(abi.FLOW_DTYPE)["hash"].copy(), torch.from_numpy(raw).cuda())


def _p(t):
    return None if t is None else ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())


def _raw_sort(engine, flows, count, idx, ws, ws_bytes):
    return engine.lib.nexg_flow_sort(engine.ctx, _p(flows), count, _p(idx), _p(ws), ws_bytes, engine._stream(None))


def test_sort_rejections(engine):
    import torch
    n = 3000
    flows = flows_from_hashes(np.arange(n, dtype=np.uint32))
    idx = torch.zeros(n + 4, dtype=torch.int32, device="cuda")
    wsb = abi.flow_sort_workspace(n)
    ws = torch.zeros(wsb // 8 + 2, dtype=torch.int64, device="cuda")
    good = dict(flows=flows, count=n, idx=idx, ws=ws, ws_bytes=wsb)
    err = lambda: engine.lib.nexg_ctx_last_error(engine.ctx)  # noqa: E731
    assert _raw_sort(engine, **good) == abi.OK
    assert _raw_sort(engine, **dict(good, ws_bytes=wsb - 1)) == abi.EINVAL
    assert b"workspace smaller than nexg_flow_sort_workspace" in err()
    assert _raw_sort(engine, **dict(good, count=1 << 32)) == abi.EINVAL
    assert b"more than 2^32 - 1 frames" in err()
    for key in ("flows", "idx", "ws"):
        assert _raw_sort(engine, **dict(good, **{key: None})) == abi.EINVAL, key
        assert b"NULL" in err()
    for key, t, step in (("flows", flows, 4), ("idx", idx, 2), ("ws", ws, 4)):
        assert _raw_sort(engine, **dict(good, **{key: t.data_ptr() + step})) == abi.EINVAL, key
        assert b"misaligned" in err()
    # count == 0 launches nothing and needs nothing
    assert _raw_sort(engine, None, 0, None, None, 0) == abi.OK
    assert engine.flow_sort(flows[:0]).numel() == 0


# ---- Engine.flow_groups ------------------------------------------------------------------------

@pytest.mark.parametrize("count", COUNTS)
def test_groups_parity_every_layout(engine, corp, count):
    which, frames = corp.tiled(count)
    for li, (lname, batch, keep) in enumerate(layouts(frames, only_first=count > 1025)):
        w = which if keep is None else which[keep]
        recs = parse_records(engine, batch)
        for oname, opt in (OPTIONS if li == 0 else OPTIONS[:2]):
            name = f"{lname} n={count} {oname}"
            flows = engine.flow(batch, recs, opt)
            groups, group_of, n, order = run_groups(engine, batch, recs, flows, opt)
            want, want_of, want_n = corp.groups(w, oname, opt)
            assert n == want_n, (name, n, want_n)
            assert (order == sort_host(corp.rows(oname, opt)["hash"][w])).all(), name
            groups_equal(groups, want, name)
            assert (group_of == want_of).all(), name
            if count >= 1023 and li == 0:
                assert (want["mixed"] > 0).sum() >= 1 and (want["packets"] > 1).sum() > 5


def test_the_collision_pair(engine):
    """Two address pairs with one hash: one group, its members interleaved,
    three changes of key among them; the same traffic from one pair only is
    one flow."""
    for pattern, mixed in (("AAAAA", 0), ("ABAAB", 3)):
        frames = fg.collision_frames(pattern)
        batch = FrameBatch.from_packed(frames, pad_to=1)
        recs = parse_records(engine, batch)
        flows = engine.flow(batch, recs)
        rows = to_host(flows, abi.FLOW_DTYPE, len(frames))
        # not vacuous: the device gives all five frames one hash, and a flow
        assert len(set(rows["hash"].tolist())) == 1 and int(rows["hash"][0]) != 0
        assert (rows["kind"] == abi.FLOW_IPV4_L4).all()
        groups, group_of, n, order = run_groups(engine, batch, recs, flows)
        assert n == 1 and order.tolist() == [0, 1, 2, 3, 4] and group_of.tolist() == [0] * 5
        g = groups[0]
        assert (int(g["packets"]), int(g["mixed"]), int(g["flags8"]) & 1) == (5, mixed, 1 if mixed else 0), pattern
        assert int(g["hash"]) == int(rows["hash"][0]) and int(g["bytes"]) == sum(len(f) for f in frames)
    # without the ports the hash is the pinned one
    ipo = to_host(engine.flow(batch, recs, FlowOption(ports=False)), abi.FLOW_DTYPE, 5)
    assert (ipo["hash"] == fg.COLLISION_HASH).all()


# fabricated batches: FLOW_IPV4 rows and records made to match (legal caller memory)

def fabricated(gid, lengths, proto=47):
    """A batch of len(gid) frames that all start at byte 0 of one 64-KiB
    buffer with the given lengths, IPv4 records whose addresses are the group
    id (so a group is one flow), flow rows with a hash that grows with the
    group id. Returns (batch, records, flows, hashes)."""
    import torch
    n = len(gid)
    recs = np.zeros(n, abi.RECORD_DTYPE)
    recs["flags"] = abi.L_ETHERNET | abi.L_IP | abi.L_IPV4
    recs["l3_off"] = 14
    recs["ip_proto"] = proto
    recs["ip_src"] = gid.astype(np.uint32)
    recs["ip_dst"] = 0x0A000001
    rows = np.zeros(n, abi.FLOW_DTYPE)
    hashes = (gid.astype(np.uint64) * 40503 + 77).astype(np.uint32)  # increasing in gid, every byte of the hash in use
    rows["hash"], rows["kind"], rows["proto"] = hashes, abi.FLOW_IPV4, proto
    batch = FrameBatch(data=torch.zeros(65536, dtype=torch.uint8, device="cuda"), count=n,
                       offsets=torch.zeros(n, dtype=torch.int64, device="cuda"),
                       lengths=torch.from_numpy(lengths.astype(np.int32)).cuda())
    return (batch, torch.from_numpy(recs.view(np.uint8).copy()).cuda(), torch.from_numpy(rows.view(np.uint8).copy()).cuda(),
            hashes)


def expected_of(lengths, hashes, proto=47):
    """(rows, group_of, order) of a fabricated batch whose groups are one flow
    each, by numpy alone: runs of the stably sorted hashes."""
    order = np.argsort(hashes, kind="stable")
    sh = hashes[order]
    head = np.ones(len(sh), bool)
    head[1:] = sh[1:] != sh[:-1]
    first = np.nonzero(head)[0]
    want = np.zeros(len(first), abi.FLOW_GROUP_DTYPE)
    want["hash"], want["kind"], want["proto"] = sh[first], abi.FLOW_IPV4, proto
    want["first"] = first
    want["packets"] = np.diff(np.append(first, len(sh)))
    want["bytes"] = np.add.reduceat(lengths[order].astype(np.uint64), first)
    want["first_index"] = order[first]
    group_of = np.zeros(len(sh), np.uint32)
    group_of[order] = np.cumsum(head) - 1
    return want, group_of, order


GROUP_SHAPES = {
    "one flow of 65793 frames": lambda n: np.zeros(n, np.int64),
    "65793 singletons": lambda n: np.arange(n, dtype=np.int64),
    # a group from the last lane of every 256-position tile to the first lane of the next
    "runs over the tile borders": lambda n: (np.arange(n, dtype=np.int64) + 1) // 2,
    # groups of 70000 frames: each spans more than 256 tiles
    "groups over more than 256 tiles": lambda n: np.arange(n, dtype=np.int64) // 70000,
}


@pytest.mark.parametrize("shape", list(GROUP_SHAPES))
def test_group_shapes(engine, shape):
    n = 140001 if "more than 256" in shape else 65793
    gid = GROUP_SHAPES[shape](n)
    if "tile borders" in shape:
        assert gid[255] == gid[256] == 128 and gid[254] != gid[255] and gid[257] != gid[256]
    lengths = 65535 - (np.arange(n) % 3)
    batch, recs, flows, hashes = fabricated(gid, lengths)
    want, want_of, want_order = expected_of(lengths, hashes)
    groups, group_of, count, order = run_groups(engine, batch, recs, flows)
    assert count == len(want) == len(np.unique(gid))
    assert (order == want_order).all() and (order == np.arange(n)).all()
    groups_equal(groups, want, shape)
    assert (group_of == want_of).all()
    assert int(groups["mixed"].sum()) == 0 and int(groups["flags8"].sum()) == 0
    # first + packets tile [0, count) exactly
    assert int(groups["first"][0]) == 0 and int(groups["first"][-1]) + int(groups["packets"][-1]) == n
    assert (groups["first"][1:] == groups["first"][:-1] + groups["packets"][:-1]).all()
    if "singletons" not in shape and "borders" not in shape:
        assert int(groups["bytes"].max()) > 1 << 32


def test_group_members_interleaved_over_the_batch(engine):
    """Frames of 300 flows dealt round-robin, two flows per hash with another
    protocol: the sort brings a group's members together in frame order and
    every second member differs from the one before it."""
    n = 60000
    flow_id = np.arange(n, dtype=np.int64) % 300
    lengths = 60 + (np.arange(n) % 1400)
    batch, recs, flows, hashes = fabricated(flow_id // 2, lengths)
    import torch
    h = to_host(recs, abi.RECORD_DTYPE, n)
    h["ip_dst"] = 0x0A000001 + (flow_id % 2)  # the two flows of a hash
    recs = torch.from_numpy(h.view(np.uint8).copy()).cuda()
    want, want_of, want_order = expected_of(lengths, hashes)
    groups, group_of, count, order = run_groups(engine, batch, recs, flows)
    assert count == 150 and (order == want_order).all() and (group_of == want_of).all()
    want["mixed"] = want["packets"] - 1
    want["flags8"] = abi.FLOW_GROUP_MIXED
    groups_equal(groups, want, "interleaved")


# ---- caps and caller memory ----------------------------------------------------------------------

def _raw_groups(engine, batch, recs, flows, opt, order, out, cap, gof, cnt, ws, ws_bytes):
    fr = batch.to_c()
    return engine.lib.nexg_flow_groups(engine.ctx, ctypes.byref(fr), _p(recs), _p(flows),
                                       None if opt is None else ctypes.byref(opt), _p(order), _p(out), cap, _p(gof),
                                       _p(cnt), _p(ws), ws_bytes, engine._stream(None))


def test_groups_cap_and_guard_words(engine, corp):
    """groups_cap 0, 1, G - 1 and G: *out_count is G every time, rows at or
    past the cap are not stored, nothing is stored behind any output, and the
    workspace's earlier contents (ones) do not matter."""
    import torch
    which, frames = corp.tiled(3000)
    batch = FrameBatch.from_packed(frames, pad_to=1)
    recs = parse_records(engine, batch)
    flows = engine.flow(batch, recs)
    order = engine.flow_sort(flows)
    want, want_of, G = corp.groups(which, *OPTIONS[0])
    n, guard = batch.count, 64
    wsb = abi.flow_groups_workspace(n)
    for cap in (0, 1, G - 1, G, G + 5):
        ws = torch.full((wsb // 8 + guard,), -1, dtype=torch.int64, device="cuda")
        out = torch.full(((cap + guard) * 32,), 0x5A, dtype=torch.uint8, device="cuda")
        gof = torch.full((n + guard,), -7, dtype=torch.int32, device="cuda")
        cnt = torch.full((1 + guard,), -7, dtype=torch.int64, device="cuda")
        assert _raw_groups(engine, batch, recs, flows, None, order, out, cap, gof, cnt, ws, wsb) == abi.OK
        torch.cuda.synchronize()
        assert int(cnt[0]) == G and bool((cnt[1:] == -7).all()), cap
        k = min(cap, G)
        groups_equal(to_host(out, abi.FLOW_GROUP_DTYPE, k), want[:k], f"cap {cap}")
        assert bool((out[k * 32:] == 0x5A).all()), cap
        assert (to_host(gof, np.uint32, n) == want_of).all() and bool((gof[n:] == -7).all()), cap
        assert bool((ws[wsb // 8:] == -1).all()), cap
    # out may be NULL with a cap of 0, out_group may be NULL
    cnt.fill_(-7)
    assert _raw_groups(engine, batch, recs, flows, None, order, None, 0, None, cnt, ws, wsb) == abi.OK
    torch.cuda.synchronize()
    assert int(cnt[0]) == G
    # Engine.flow_groups with a capacity: one call, the rows that fit
    groups, group_of, got_n, _ = engine.flow_groups(batch, recs, flows, groups_cap=7)
    assert got_n == G and groups.numel() == 7 * 32
    groups_equal(to_host(groups, abi.FLOW_GROUP_DTYPE, 7), want[:7], "groups_cap=7")


def test_arbitrary_flows_and_order(engine, corp):
    """flows with every byte random, and an order with entries past the batch
    and duplicates: the rows are groups_host's on the same arrays (group
    numbers are defined for a permutation only), nothing faults, nothing is
    stored outside the outputs."""
    import torch
    which, frames = corp.tiled(5000)
    batch = FrameBatch.from_packed(frames, pad_to=1)
    recs = parse_records(engine, batch)
    n, guard = batch.count, 64
    rng = np.random.default_rng(21)
    raw = rng.integers(0, 256, n * 8, dtype=np.uint8)
    raw.view(abi.FLOW_DTYPE)["hash"][::3] &= 0x3  # some runs of equal hashes
    flows_h = raw.view(abi.FLOW_DTYPE).copy()
    flows = torch.from_numpy(raw).cuda()
    order_h = sort_host(flows_h["hash"])
    order_h[10:4000:7] = order_h[9:3999:7]          # duplicates
    order_h[5:4000:11] = n + rng.integers(0, 1 << 31, len(order_h[5:4000:11]))  # past the batch
    order_h[-1] = 0xFFFFFFFF
    order_h[0] = n
    order = torch.from_numpy(order_h.view(np.int32).copy()).cuda()
    for oname, opt in OPTIONS[:2]:
        want, _, G = corp.groups(which, oname, opt, order=order_h, flows=flows_h)
        wsb = abi.flow_groups_workspace(n)
        ws = torch.full((wsb // 8 + guard,), -1, dtype=torch.int64, device="cuda")
        out = torch.full(((G + guard) * 32,), 0x5A, dtype=torch.uint8, device="cuda")
        gof = torch.full((n + guard,), -7, dtype=torch.int32, device="cuda")
        cnt = torch.full((1 + guard,), -7, dtype=torch.int64, device="cuda")
        assert _raw_groups(engine, batch, recs, flows, opt.to_c(), order, out, G, gof, cnt, ws, wsb) == abi.OK
        torch.cuda.synchronize()
        assert int(cnt[0]) == G and bool((cnt[1:] == -7).all())
        groups_equal(to_host(out, abi.FLOW_GROUP_DTYPE, G), want, f"hostile {oname}")
        assert bool((out[G * 32:] == 0x5A).all()) and bool((gof[n:] == -7).all()) and bool((ws[wsb // 8:] == -1).all())
        named = np.zeros(n, bool)
        named[order_h[order_h < n]] = True
        assert (to_host(gof, np.int32, n)[~named] == -7).all()  # a frame the order leaves out gets no store


def test_hostile_records(engine, corp):
    """Records are caller memory, as in tests/test_gpu_flow.py: l3_off at, just
    past and far past the frame, a claimed IPv6 layer on a frame without one,
    and an IPv6 header that ends on the data's last byte. The keys, and so
    `mixed`, are groups_host's on the same records."""
    import torch
    base = [f for f in corp.frames if len(f) < 2000]
    v6 = next(x.frame for x in ff.corpus() if x.what == "vector 5 udp")
    frames = (base * 5)[:299] + [v6]
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
    last = len(frames) - 1
    h["l3_off"][last] = len(v6) - 40  # ends exactly on the last byte of the data
    h["flags"][last] = abi.L_ETHERNET | abi.L_IP | abi.L_IPV6
    dev = torch.from_numpy(h.view(np.uint8).copy()).cuda()
    lengths = [len(f) for f in frames]
    # the honest rows: hostile records then change keys under unchanged hashes
    flows = engine.flow(batch, recs)
    flows_h = to_host(flows, abi.FLOW_DTYPE, len(frames))
    for opt in (FlowOption(), FlowOption(symmetric=True)):
        want, want_of, G = groups_host(frames, h, lengths, flows_h, opt)
        groups, group_of, n, order = run_groups(engine, batch, dev, flows, opt)
        assert n == G and (group_of == want_of).all()
        groups_equal(groups, want, "hostile records")
        assert (want["mixed"] > 0).sum() > 3


def test_groups_are_deterministic(engine, corp):
    import torch
    which, frames = corp.tiled(65793)
    batch = FrameBatch.from_packed(frames, pad_to=1)
    recs = parse_records(engine, batch)
    flows = engine.flow(batch, recs)
    runs = []
    for _ in range(2):
        groups, group_of, n, order = engine.flow_groups(batch, recs, flows)
        runs.append((groups.clone(), group_of.clone(), order.clone(), n))
    for a, b in zip(*runs):
        assert a == b if isinstance(a, int) else torch.equal(a, b)


def test_groups_rejections(engine, corp):
    import torch
    which, frames = corp.tiled(300)
    batch = FrameBatch.from_packed(frames, pad_to=1)
    recs = parse_records(engine, batch)
    flows = engine.flow(batch, recs)
    order = engine.flow_sort(flows)
    n = batch.count
    wsb = abi.flow_groups_workspace(n)
    ws = torch.zeros(wsb // 8 + 2, dtype=torch.int64, device="cuda")
    out = torch.zeros((n + 2) * 32, dtype=torch.uint8, device="cuda")
    gof = torch.zeros(n + 4, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    good = dict(recs=recs, flows=flows, opt=None, order=order, out=out, cap=n, gof=gof, cnt=cnt, ws=ws, ws_bytes=wsb)
    err = lambda: engine.lib.nexg_ctx_last_error(engine.ctx)  # noqa: E731
    assert _raw_groups(engine, batch, **good) == abi.OK
    assert _raw_groups(engine, batch, **dict(good, opt=FlowOption(flags=0x8).to_c(validate=False))) == abi.EINVAL
    assert b"unknown flag bits" in err()
    assert _raw_groups(engine, batch, **dict(good, opt=FlowOption(reserved=1).to_c(validate=False))) == abi.EINVAL
    assert b"reserved must be 0" in err()
    assert _raw_groups(engine, batch, **dict(good, ws_bytes=wsb - 1)) == abi.EINVAL
    assert b"workspace smaller than nexg_flow_groups_workspace" in err()
    for key in ("recs", "flows", "order", "out", "cnt", "ws"):
        assert _raw_groups(engine, batch, **dict(good, **{key: None})) == abi.EINVAL, key
        assert b"NULL" in err()
    for key, t, step in (("recs", recs, 8), ("out", out, 8), ("flows", flows, 4), ("cnt", cnt, 4), ("ws", ws, 4),
                         ("order", order, 2), ("gof", gof, 2)):
        assert _raw_groups(engine, batch, **dict(good, **{key: t.data_ptr() + step})) == abi.EINVAL, key
        assert b"misaligned" in err()
    # an invalid frame table: offsets without data
    bad = batch.to_c()
    bad.data = None
    assert engine.lib.nexg_flow_groups(engine.ctx, ctypes.byref(bad), _p(recs), _p(flows), None, _p(order), _p(out), n,
                                       _p(gof), _p(cnt), _p(ws), wsb, engine._stream(None)) == abi.EINVAL
    assert b"invalid frame batch" in err()
    # more than 2^32 - 1 frames (refused before anything is read)
    huge = FrameBatch(data=batch.data, count=1 << 32, stride=0, offsets=batch.offsets)
    assert _raw_groups(engine, huge, **good) == abi.EINVAL
    assert b"2^32 - 1" in err() or b"invalid frame batch" in err()
    with pytest.raises(ValueError):
        engine.flow_groups(batch, recs, flows, FlowOption(flags=0x10))
    # count == 0 writes *out_count = 0 and needs nothing else
    cnt.fill_(7)
    empty = FrameBatch.from_packed([], pad_to=1)
    assert _raw_groups(engine, empty, None, None, None, None, None, 0, None, cnt, None, 0) == abi.OK
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [0, 7, 7, 7]
    groups, group_of, k, order0 = engine.flow_groups(empty, recs[:0], flows[:0])
    assert k == 0 and groups.numel() == 0 and group_of.numel() == 0 and order0.numel() == 0


# ---- composition -----------------------------------------------------------------------------------

def test_first_records_and_buckets(engine, corp):
    """gather_rows(records, 64, groups.first_index) gives each flow's first
    record; the groups of a flow_partition bucket are the whole batch's groups
    with hash % buckets == b, with equal counters."""
    import torch
    which, frames = corp.tiled(2000)
    batch = FrameBatch.from_packed(frames, pad_to=1)
    recs = parse_records(engine, batch)
    flows = engine.flow(batch, recs)
    groups_d, group_of, n, order = engine.flow_groups(batch, recs, flows)
    groups = to_host(groups_d, abi.FLOW_GROUP_DTYPE, n)
    first_index = groups_d.view(torch.int32).view(-1, 8)[:, 7].contiguous()
    assert (to_host(first_index, np.uint32, n) == groups["first_index"]).all()
    first_recs = to_host(engine.gather_rows(recs, 64, first_index), abi.RECORD_DTYPE, n)
    assert first_recs.tobytes() == to_host(recs, abi.RECORD_DTYPE, batch.count)[groups["first_index"]].tobytes()
    buckets = 8
    idx, table, first = engine.flow_partition(batch, flows, buckets)
    hidx = to_host(idx, np.uint32, batch.count)
    seen = 0
    for b in range(buckets):
        lo, hi = int(first[b]), int(first[b + 1])
        part = engine.flow_bucket(table, first, b)
        rec_b = engine.gather_rows(recs, 64, idx[lo:hi])
        flows_b = engine.gather_rows(flows, 8, idx[lo:hi])
        got, _, k, _ = run_groups(engine, part, rec_b, flows_b)
        want = groups[groups["hash"] % buckets == b]
        assert k == len(want) > 0, b
        for f in ("hash", "kind", "proto", "flags8", "packets", "bytes", "mixed"):
            assert (got[f] == want[f]).all(), (b, f)
        assert (hidx[lo:hi][got["first_index"]] == want["first_index"]).all(), b
        seen += k
    assert seen == n


def test_cpp_flow_groups_gpu(oracle, tmp_path):
    exe = build_native_test("cpp_flow_groups_test")
    frames = [x.frame for x in ff.small_corpus()] + fg.collision_frames()
    recs = oracle.parse_frames(frames, ff.PARSE_FLAGS)
    lengths = [len(f) for f in frames]
    p = tmp_path / "frames.txt"
    p.write_text("".join((f.hex() or "-") + "\n" for f in frames))
    r = subprocess.run([exe, "--gpu", str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    it = iter(l.split() for l in r.stdout.splitlines())
    for oi, opt in enumerate((FlowOption(), FlowOption(symmetric=True))):
        flows = flows_host(frames, recs, lengths, opt)
        want, want_of, n = groups_host(frames, recs, lengths, flows, opt)
        assert next(it) == ["O", str(oi), str(len(frames)), str(n)]
        for g in want:
            assert next(it) == ["G", f"{int(g['hash']):08x}"] + [str(int(g[f])) for f in GROUP_FIELDS if f not in
                                                                  ("hash", "reserved")], (oi, g)
        assert next(it) == ["I"] + [str(i) for i in sort_host(flows["hash"])], oi
        assert next(it) == ["M"] + [str(i) for i in want_of], oi
    assert next(it, None) is None
