"""GPU: the flow table across batches (nexg_flow_table_merge, Engine.flow_table_merge, FlowTable).

The expectation is nex_amd.flow.merge_host (checked against the independent
per-hash dictionary of tests/flow_table_ref.py in tests/test_flow_table_host.py),
and for the whole pipeline that dictionary itself. Fabricated merges need no
frames: the frame table is empty and every group's first_index is past it, so
its key is the key of a frame without a flow; a made-up entry with that key
matches cleanly and one with any other key turns MIXED.

Shapes: sizes around a wave and a 256-position tile for both inputs and every
pair of them; a 2049-position merge whose every tile border falls between an
entry and its group; 105793 positions = 414 tiles, so the one-workgroup scan of
the tile totals carries; capacities 0, n_out - 1 and n_out; the batch sequences
of the CPU tests (collisions, hash 0, expiry); the corpus in every frame-table
layout through FlowTable from capacity 1; inputs that are not ascending. Every
call runs with guard words behind each output and the workspace."""
import ctypes

import numpy as np
import pytest

from nex_amd import abi
from nex_amd.engine import FlowTable, FrameBatch
from nex_amd.flow import FlowOption, flows_host, groups_host, merge_host
from tests import flow_table_ref as tr
from tests.helpers import layouts, parse_records, to_host

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1025]
GUARD = 64
_p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def raw_merge(engine, groups, table, epoch=0, min_epoch=0, cap=None, batch=None, recs=None, opt=None, slots=True):
    """One call of the C entry on host arrays with guard words behind every
    output and the workspace: (the rows stored, *out_count, out_slot)."""
    import torch
    n_in, n_g = len(table), len(groups)
    cap = n_in + n_g if cap is None else cap
    batch = FrameBatch.from_packed([], pad_to=1) if batch is None else batch
    fr = batch.to_c()
    t_in, g = dev(table) if n_in else None, dev(groups) if n_g else None
    out = torch.full(((cap + GUARD) * 64,), 0x5A, dtype=torch.uint8, device="cuda")
    slot = torch.full((n_g + GUARD,), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((1 + GUARD,), -7, dtype=torch.int64, device="cuda")
    wsb = abi.flow_table_workspace(n_in, n_g)
    ws = torch.full((wsb // 8 + GUARD,), -1, dtype=torch.int64, device="cuda")
    rc = engine.lib.nexg_flow_table_merge(engine.ctx, ctypes.byref(fr), _p(recs), None if opt is None else ctypes.byref(opt),
                                          _p(g), n_g, _p(t_in), n_in, epoch, min_epoch, _p(out), cap,
                                          _p(slot) if slots else None, _p(cnt), _p(ws), wsb, engine._stream(None))
    assert rc == abi.OK, engine.lib.nexg_ctx_last_error(engine.ctx)
    torch.cuda.synchronize()
    n_out = int(cnt[0])
    k = min(cap, n_out)
    assert bool((cnt[1:] == -7).all()) and bool((out[k * 64:] == 0x5A).all()) and bool((ws[wsb // 8:] == -1).all())
    assert bool((slot[n_g:] == -7).all()) and (slots or bool((slot == -7).all()))
    return to_host(out, abi.FLOW_ENTRY_DTYPE, k), n_out, to_host(slot, np.uint32, n_g)


def made_up_table(hashes, rng):
    """Entries with these hashes: half hold the key of a frame without a flow,
    half some other key; MIXED here and there; last_epoch 0..9."""
    t = np.zeros(len(hashes), abi.FLOW_ENTRY_DTYPE)
    t["hash"] = hashes
    other = rng.random(len(t)) < 0.5
    t["kind"] = np.where(other, rng.integers(0, 5, len(t)), 0)
    t["proto"] = np.where(other, rng.integers(0, 256, len(t)), 0)
    t["key"] = np.where(other[:, None], rng.integers(0, 256, (len(t), 36)), 0)
    t["key"][other & (t["kind"] == 0) & (t["proto"] == 0), 5] |= 1  # "other" is never the no-flow key
    t["flags8"] = rng.random(len(t)) < 0.2
    t["last_epoch"] = rng.integers(0, 10, len(t))
    t["packets"] = rng.integers(1, 1 << 40, len(t))
    t["bytes"] = rng.integers(0, 1 << 50, len(t))
    return t


def made_up_groups(hashes, rng, first_index_from=0):
    """Group rows with these hashes whose first_index is at or past `first_index_from`."""
    g = np.zeros(len(hashes), abi.FLOW_GROUP_DTYPE)
    g["hash"] = hashes
    g["kind"], g["proto"] = rng.integers(0, 5, len(g)), rng.integers(0, 256, len(g))
    g["mixed"] = np.where(rng.random(len(g)) < 0.2, rng.integers(1, 9, len(g)), 0)
    g["flags8"] = g["mixed"] != 0
    g["first"] = rng.integers(0, 1 << 20, len(g))
    g["packets"] = rng.integers(1, 1 << 32, len(g))
    g["bytes"] = rng.integers(0, 1 << 47, len(g))
    g["first_index"] = rng.integers(first_index_from, 1 << 32, len(g))
    if len(g):
        g["first_index"][0] = first_index_from
    return g


def check_made_up(engine, table_hashes, group_hashes, rng, name, epoch=11, min_epoch=5, **kw):
    table, groups = made_up_table(np.sort(table_hashes), rng), made_up_groups(np.sort(group_hashes), rng)
    want, want_slot = merge_host(table, groups, [], [], [], FlowOption(), epoch, min_epoch)
    got, n_out, slot = raw_merge(engine, groups, table, epoch, min_epoch, **kw)
    assert n_out == len(want), (name, n_out, len(want))
    tr.entries_equal(got, want, name)
    assert (slot == want_slot).all(), name
    return got, slot


def hash_sets(rng, n_in, n_groups):
    """Distinct random hashes for both sides, about half of the smaller side
    shared; 0 leads and 0xFFFFFFFF ends every side that has room for it."""
    mid = np.unique(rng.integers(1, 0xFFFFFFFF, 2 * (n_in + n_groups) + 8, dtype=np.uint64).astype(np.uint32))
    rng.shuffle(mid)
    shared = min(n_in, n_groups) // 2
    a, b = mid[:n_in].copy(), np.concatenate([mid[:shared], mid[n_in: n_in + n_groups - shared]])
    for x in (a, b):
        x[:1] = 0
        if len(x) >= 2:
            x[-1] = 0xFFFFFFFF
    if n_in == n_groups == 1:
        b[0] = 0xFFFFFFFF
    return a, b


@pytest.mark.parametrize("n_in", SIZES)
def test_sizes(engine, n_in):
    rng = np.random.default_rng(100 + n_in)
    for n_groups in SIZES:
        a, b = hash_sets(rng, n_in, n_groups)
        assert len(a) == n_in and len(b) == n_groups and len(set(a)) == n_in and len(set(b)) == n_groups
        assert n_in + n_groups < 2 or {0, 0xFFFFFFFF} <= set(a.tolist()) | set(b.tolist())
        check_made_up(engine, a, b, rng, f"{n_in} x {n_groups}")


def test_patterns(engine):
    rng = np.random.default_rng(7)
    h = np.unique(rng.integers(1, 1 << 32, 1300, dtype=np.uint64).astype(np.uint32))[:1200]
    for name, a, b in (("disjoint", h[:600], h[600:]), ("identical", h[:700], h[:700]), ("interleaved", h[::2], h[1::2]),
                       ("table below groups", h[:500], h[500:]), ("groups below table", h[700:], h[:700]),
                       ("one entry in the middle", h[600:601], h), ("one group in the middle", h, h[600:601]),
                       ("one matching group", h, h[-1:]), ("one matching entry", h[:1], h)):
        for min_epoch in (0, 5, 100):
            check_made_up(engine, a, b, rng, f"{name} min_epoch {min_epoch}", min_epoch=min_epoch)


def test_every_tile_border_between_an_entry_and_its_group(engine):
    """2049 merged positions; at each of the 8 tile borders the entry is
    position 256 k - 1 and its group position 256 k. Elsewhere lone entries,
    lone groups and pairs at random."""
    rng = np.random.default_rng(8)
    n, kinds, p = 2049, [], 0
    border = {256 * k - 1 for k in range(1, 9)}
    while p < n:
        if p in border:
            kinds.append("pair")
        elif p + 1 in border or p + 1 == n:
            kinds.append(rng.choice(["a", "b"]))
        else:
            kinds.append(rng.choice(["a", "b", "pair"]))
            if kinds[-1] == "pair" and p + 2 in border:
                kinds[-1] = "a"
        p += 2 if kinds[-1] == "pair" else 1
    assert p == n
    h = np.cumsum(rng.integers(1, 1000, len(kinds))).astype(np.uint32)
    a = h[[k in ("a", "pair") for k in kinds]]
    b = h[[k in ("b", "pair") for k in kinds]]
    assert len(a) + len(b) == n
    # positions of the merged order (ties: the entry first): every border pair straddles a tile border
    merged = sorted([(int(x), 0) for x in a] + [(int(x), 1) for x in b])
    for k in range(1, 9):
        assert merged[256 * k - 1][0] == merged[256 * k][0] and merged[256 * k - 1][1] == 0
    for min_epoch in (0, 5, 100):
        check_made_up(engine, a, b, rng, f"borders min_epoch {min_epoch}", min_epoch=min_epoch)


def test_more_than_256_tiles_and_determinism(engine):
    """65793 entries and 40000 groups, half of the groups' hashes shared: 414
    tiles, so the scan of the tile totals carries. A second run is bit-equal."""
    rng = np.random.default_rng(9)
    pool = np.unique(rng.integers(0, 1 << 32, 120000, dtype=np.uint64).astype(np.uint32))
    rng.shuffle(pool)
    a, b = pool[:65793], np.concatenate([pool[:20000], pool[65793: 85793]])
    table, groups = made_up_table(np.sort(a), rng), made_up_groups(np.sort(b), rng)
    want, want_slot = merge_host(table, groups, [], [], [], FlowOption(), 11, 5)
    got, n_out, slot = raw_merge(engine, groups, table, 11, 5)
    assert n_out == len(want) and 20000 < n_out < 85793
    tr.entries_equal(got, want, "414 tiles")
    assert (slot == want_slot).all()
    again, n_again, slot_again = raw_merge(engine, groups, table, 11, 5)
    assert n_again == n_out and again.tobytes() == got.tobytes() and slot_again.tobytes() == slot.tobytes()


def test_capacity(engine):
    rng = np.random.default_rng(10)
    a, b = hash_sets(rng, 700, 900)
    table, groups = made_up_table(np.sort(a), rng), made_up_groups(np.sort(b), rng)
    want, want_slot = merge_host(table, groups, [], [], [], FlowOption(), 11, 5)
    n_out = len(want)
    assert 900 < n_out < 1600
    for cap in (0, 1, n_out - 1, n_out, n_out + 3):
        got, n, slot = raw_merge(engine, groups, table, 11, 5, cap=cap)  # the guards behind the cap are checked there
        assert n == n_out and len(got) == min(cap, n_out), cap
        tr.entries_equal(got, want[: len(got)], f"cap {cap}")
        assert (slot == want_slot).all(), cap
    got, n, _ = raw_merge(engine, groups, table, 11, 5, slots=False)  # out_slot is optional
    assert n == n_out
    tr.entries_equal(got, want, "no out_slot")


def device_batch(b):
    """A tests.flow_table_ref.Batch on the device: (FrameBatch, records)."""
    import torch
    batch = FrameBatch.from_frames(b.frames, pad_to=4)
    recs = torch.from_numpy(b.recs.view(np.uint8).reshape(-1).copy()).cuda()
    return batch, recs


@pytest.mark.parametrize("symmetric,ports", [(False, True), (True, False)])
def test_the_cpu_sequences_on_the_device(engine, oracle, symmetric, ports):
    """Collisions across batches, the no-flow entry, keys that differ in kind
    or protocol alone, expiry at, below and above min_epoch, empty batches:
    Engine.flow_groups + Engine.flow_table_merge on the oracle's records and
    the sequences' flow rows, against merge_host and the dictionary. (The
    sequence with bad extents stays on the CPU: its frames have no bytes.)"""
    option = tr.option_of(symmetric, ports)
    for name, batches in tr.sequences(oracle).items():
        if name == "bad extents":
            continue
        want_ref, _ = tr.run_reference(batches, symmetric, ports)
        want_host = tr.run_host(merge_host, batches, symmetric, ports)
        table = None
        for k, b in enumerate(batches):
            batch, recs = device_batch(b)
            flows = dev(b.flows(symmetric, ports))
            groups, group_of, _, _ = engine.flow_groups(batch, recs, flows, option)
            table, n_out, slot = engine.flow_table_merge(batch, recs, groups, table, b.epoch, b.min_epoch, option)
            got = to_host(table, abi.FLOW_ENTRY_DTYPE, n_out)
            tr.entries_equal(got, want_host[k][0], (name, k, "merge_host"))
            tr.entries_equal(got, want_ref[k][0], (name, k, "reference"))
            row = to_host(slot, np.uint32, slot.numel())[to_host(group_of, np.uint32, batch.count)]
            assert (row == want_ref[k][1]).all(), (name, k)


class Pipeline:
    """The corpus with the collision pair tiled to three batches, the oracle's
    records, and per option the expected tables (computed once per option and
    per set of frames kept)."""
    COUNTS = (65, 257, 1025)

    def __init__(self, oracle):
        from tests import flow_frames as ff
        self.frames = tr.corpus_frames()
        self.recs = oracle.parse_frames(self.frames, ff.PARSE_FLAGS)
        self.lengths = np.array([len(f) for f in self.frames])
        n = len(self.frames)
        self.which = [(np.arange(c) + 41 * k) % n for k, c in enumerate(self.COUNTS)]
        self.flows, self.want = {}, {}

    def expected(self, symmetric, ports, small):
        """Per batch (merge_host's table, the dictionary's rows, the row of
        every frame); small: without the frames of 4096 bytes or more."""
        key = (symmetric, ports, small)
        if key not in self.want:
            option = tr.option_of(symmetric, ports)
            if (symmetric, ports) not in self.flows:
                self.flows[(symmetric, ports)] = flows_host(self.frames, self.recs, self.lengths, option)
            rows = self.flows[(symmetric, ports)]
            table, refd, out = np.zeros(0, abi.FLOW_ENTRY_DTYPE), tr.RefTable(symmetric, ports), []
            for epoch, w in enumerate(self.which):
                w = w[self.lengths[w] < 4096] if small else w
                frames = [self.frames[i] for i in w]
                groups, group_of, _ = groups_host(frames, self.recs[w], self.lengths[w], rows[w], option)
                table, slot = merge_host(table, groups, frames, self.recs[w], self.lengths[w], option, epoch, 0)
                refd.feed(frames, self.recs[w], self.lengths[w], rows["hash"][w], epoch, 0)
                assert (slot[group_of] == refd.row_of(rows["hash"][w])).all()
                out.append((table, refd.rows(), slot[group_of]))
            self.want[key] = out
        return self.want[key]


@pytest.fixture(scope="module")
def pipe(oracle):
    return Pipeline(oracle)


@pytest.mark.parametrize("symmetric,ports", [(False, True), (True, True)])
def test_whole_pipeline_in_every_layout(engine, pipe, symmetric, ports):
    option = tr.option_of(symmetric, ports)
    per_batch = [layouts([pipe.frames[i] for i in w]) for w in pipe.which]
    for li in range(len(per_batch[0])):
        lname = per_batch[0][li][0]
        table = FlowTable(engine, option, capacity=1)  # every update has to grow it
        want = pipe.expected(symmetric, ports, small=per_batch[0][li][2] is not None)
        for epoch, per_layout in enumerate(per_batch):
            _, batch, keep = per_layout[li]
            slot, group_of = table.update(batch, parse_records(engine, batch), epoch)
            got = table.rows()
            tr.entries_equal(got, want[epoch][0], (lname, epoch, "merge_host"))
            tr.entries_equal(got, want[epoch][1], (lname, epoch, "reference"))
            row = to_host(slot, np.uint32, slot.numel())[to_host(group_of, np.uint32, batch.count)]
            assert (row == want[epoch][2]).all(), (lname, epoch)
            assert table.count == len(got) <= table.capacity
        assert int(got["packets"].sum()) == sum(b[li][1].count for b in per_batch), lname
        assert int(got["flags8"].sum()) >= 1, lname  # the collision pair


def test_inputs_that_are_not_ascending(engine, pipe):
    """A shuffled table_in, and groups in any order with any first_index (real
    frames, frames past the batch), packets and flags8: the result is
    unspecified, the stores are not. raw_merge checks the guard words behind
    table_out, out_slot, *out_count and the workspace."""
    rng = np.random.default_rng(12)
    w = pipe.which[1]
    w = w[pipe.lengths[w] < 4096]
    batch = FrameBatch.from_packed([pipe.frames[i] for i in w], pad_to=1)
    recs = parse_records(engine, batch)
    for n_in, n_g in ((1000, 1300), (257, 0), (0, 513), (5, 3000)):
        a = rng.integers(0, 1 << 32, n_in, dtype=np.uint64).astype(np.uint32)
        b = rng.integers(0, 1 << 32, n_g, dtype=np.uint64).astype(np.uint32)
        a[::5], b[::7] = 7, 7  # runs of equal hashes as well
        table, groups = made_up_table(a, rng), made_up_groups(b, rng)
        groups["first_index"][::2] = rng.integers(0, batch.count, len(groups["first_index"][::2]))
        for cap in (n_in + n_g, 100):
            _, n_out, _ = raw_merge(engine, groups, table, 11, 5, cap=cap, batch=batch, recs=recs)
            assert 0 <= n_out <= n_in + n_g
