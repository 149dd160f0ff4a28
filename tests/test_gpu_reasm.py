"""GPU: IPv4 reassembly (nexg_reasm_plan, nexg_reasm_frames, nexg_reasm_held;
nex_amd.reassemble.Reassembler).

Every output byte, pads included, the output table (offsets, lengths, source
index), the rows and the held table must equal
nex_amd.reassemble.reassemble_host(exact=False) exactly (which
tests/test_reasm_host.py pins from outside). Shapes: the corpus of
tests/reasm_frames.py in every table form of tests.helpers.layouts, align 1
and 16; input counts around a workgroup of the fill (16 frames), a plan tile
(256) and 4097; the 8183-piece train spread over workgroups and tiles; a
destination pre-filled with 0xA5 and two runs; the collision rows; fragment ->
shuffle -> reassemble on the IMIX batch; encap -> fragment -> shuffle ->
reassemble -> parse -> decap; a per-frame row carried through by gather_rows;
push over three batches with an epoch timeout."""
import ctypes
import functools
import random

import numpy as np
import pytest

from nex_amd import abi
from nex_amd.encap import Tunnel, TunnelSet
from nex_amd.engine import FrameBatch
from nex_amd.fragment import fragment_host
from nex_amd.reassemble import Reassembler, pack_host, reassemble_host
from tests import fragment_frames as ff
from tests import helpers
from tests import reasm_frames as rf

pytestmark = pytest.mark.gpu

FILL = 0xA5
COUNTS = (1, 15, 16, 17, 255, 256, 257, 4097)


@functools.lru_cache(maxsize=None)
def corpus_table():
    """The corpus cases under 2100 bytes a frame, without the bad extents (test_extents_that_leave_the_data)."""
    return tuple(f for f in rf.table(2100)[0] if f is not None)


def want_of(frames, align):
    out, src, rows, collided = reassemble_host(frames, align, exact=False)
    data, offs = pack_host(out, align)
    return out, src, rows, np.frombuffer(data, np.uint8), offs


def check(engine, name, batch, want, align, rs=None):
    """Reassembler.run of `batch` against want_of()."""
    import torch
    out_frames, src, rows, buf, offs = want
    out, d_src, d_rows, (hidx, held) = (rs or Reassembler(engine)).run(batch, align)
    torch.cuda.synchronize()
    got_rows = helpers.to_host(d_rows, abi.REASM_DTYPE, batch.count)
    bad = np.nonzero((got_rows.view(np.uint8).reshape(-1, 16) != rows.view(np.uint8).reshape(-1, 16)).any(axis=1))[0]
    assert len(bad) == 0, (name, int(bad[0]), got_rows[bad[0]], rows[bad[0]], len(bad))
    assert out.count == len(out_frames) and out.data.numel() == len(buf), (name, out.count, len(out_frames), out.data.numel(), len(buf))
    assert (out.offsets.cpu().numpy() == offs).all(), name
    assert d_src.dtype == torch.int32 and (d_src.cpu().numpy().view(np.uint32) == src).all(), name
    if align == 1:
        assert out.lengths is None
    else:
        assert (out.lengths.cpu().numpy() == [len(p) for p in out_frames]).all(), name
        assert out.hints == abi.FRAMES_MONOTONE
    got = out.data.cpu().numpy()
    if not (got == buf).all():
        b = int(np.nonzero(got != buf)[0][0])
        k = int(np.searchsorted(offs, b, side="right")) - 1
        raise AssertionError(f"{name}: byte {b} (output frame {k} of input {src[k]}, at {b - int(offs[k])} of "
                             f"{len(out_frames[k])}) is {got[b]}, want {buf[b]}")
    want_held = np.flatnonzero(rows["kind"] == abi.REASM_HELD)
    assert held.count == len(want_held) and (hidx.cpu().numpy().view(np.uint32) == want_held).all(), name
    return out, d_src, d_rows, (hidx, held)


@pytest.mark.parametrize("align", (1, 16))
def test_corpus_in_every_table_form(engine, align):
    frames = list(corpus_table())
    kinds, forms = set(), set()
    for name, batch, keep in helpers.layouts(frames, strided_below=700):
        sub = frames if keep is None else [frames[i] for i in keep]
        want = want_of(sub, align)
        kinds |= set(want[2]["kind"])
        check(engine, f"align {align} {name}", batch, want, align)
        forms.add((batch.offsets is None, batch.lengths is None, bool(batch.hints & abi.FRAMES_OFFSETS32)))
    assert kinds == {abi.REASM_PASS, abi.REASM_HEAD, abi.REASM_PART, abi.REASM_HELD}
    assert forms >= {(True, False, False), (False, True, False), (False, False, False), (False, True, True), (False, False, True)}


def test_the_64_kib_trains(engine):
    """hl + D at 65535 and 65536, and the long frames of the fragment corpus, at two phases."""
    frames = [f for name, _, fs in rf.cases() if "6553" in name or name == "the long frames, shuffled" for f in fs]
    want = want_of(frames, 1)
    assert sorted(len(f) for f in want[0])[-4:] == [65535] + [14 + 65535] * 3 and (want[2]["kind"] == abi.REASM_HELD).sum() == 4
    check(engine, "64 KiB from byte 1", helpers.packed_from_byte_1(frames), want, 1)
    check(engine, "64 KiB align 16", FrameBatch.from_packed(frames, pad_to=1, shift=4), want_of(frames, 16), 16)


@pytest.mark.parametrize("align", (1, 16))
def test_extents_that_leave_the_data(engine, align):
    frames = [f for name, _, fs in rf.cases() if name.startswith(("mtu 576", "mtu 1500")) for f in fs][:600]
    batch = FrameBatch.from_frames(frames)
    nbytes = batch.data.numel()
    boff, blen = batch.offsets.clone(), batch.lengths.clone()
    for n, k in enumerate(range(3, len(frames), 11)):
        kind = n % 5
        if kind == 0:
            boff[k] = nbytes + 1
        elif kind == 1:
            boff[k] = (1 << 62) + 5
        elif kind == 2:
            blen[k] = 65536
        elif kind == 3:
            blen[k] = -1  # 0xFFFFFFFF
        else:
            boff[k], blen[k] = nbytes - 7, 8  # ends one byte past the data
        frames[k] = None
    want = want_of(frames, align)
    assert int((want[2]["status"] == abi.ERR_BAD_EXTENT).sum()) >= 5 and (want[2]["kind"] == abi.REASM_HEAD).any()
    for hints in (0, abi.FRAMES_MONOTONE):
        bad = FrameBatch(data=batch.data, count=batch.count, offsets=boff, lengths=blen, hints=hints)
        check(engine, f"bad extents align {align} hints {hints}", bad, want, align)


@pytest.mark.parametrize("align", (1, 16))
@pytest.mark.parametrize("count", COUNTS)
def test_counts(engine, count, align):
    """The group and tile edges: 16 input frames per workgroup of the fill, 256
    per tile of the plan and of the marks, 1024 per tile of the sort."""
    pool = list(corpus_table())
    random.Random(7).shuffle(pool)
    pool = pool[5000:5000 + 4097] if count > 257 else [f for _, _, fs in rf.cases()[-12:] for f in fs if f is not None and len(f) < 2100]
    frames = [pool[i % len(pool)] for i in range(count)]
    want = want_of(frames, align)
    check(engine, f"n={count} align {align}", helpers.packed_from_byte_1(frames), want, align)


@functools.lru_cache(maxsize=None)
def spread_train():
    """The 8183-piece train shuffled among 3000 other frames: its head and its
    parts sit in different workgroups of the fill and tiles of the plan."""
    rng = random.Random(11)
    frames = list(rf.long_train()) + [f for f in corpus_table() if len(f) < 200][:3000]
    rng.shuffle(frames)
    return tuple(frames)


def test_the_8183_piece_train_spread_over_workgroups_and_tiles(engine):
    frames = list(spread_train())
    want = want_of(frames, 1)
    head = int(np.flatnonzero(want[2]["members"] == 8183)[0])
    parts = np.flatnonzero(want[2]["head"] == head)
    assert len(parts) == 8183 and len(set(parts // 16)) > 500 and len(set(parts // 256)) > 40
    check(engine, "8183 pieces", FrameBatch.from_packed(frames, pad_to=1, shift=4), want, 1)
    check(engine, "8183 pieces, align 16", helpers.packed_from_byte_1(frames), want_of(frames, 16), 16)


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("align", (1, 16))
def test_prefilled_destination_and_two_runs(engine, align):
    """Nothing is stored outside the outputs, the pads are zero, the tables have
    no entry past their counts, and a second run gives the same bits."""
    import torch
    frames = list(corpus_table()[2000:2000 + 1500])
    n = len(frames)
    out_frames, src, rows, buf, offs = want_of(frames, align)
    total, k = len(buf), len(out_frames)
    batch = helpers.packed_from_byte_1(frames)
    fr = batch.to_c()
    runs = []
    for _ in range(2):
        first = torch.full((n + 3,), -1, dtype=torch.int32, device="cuda")
        nbytes = torch.full((n + 3,), -1, dtype=torch.int64, device="cuda")
        d_rows = torch.full(((n + 2) * 16,), FILL, dtype=torch.uint8, device="cuda")
        ws_bytes = abi.reasm_plan_workspace(n)
        ws = torch.full((ws_bytes + 64,), FILL, dtype=torch.uint8, device="cuda")
        rc = engine.lib.nexg_reasm_plan(engine.ctx, ctypes.byref(fr), align, P(first), P(nbytes), P(d_rows), P(ws), ws_bytes,
                                        engine._stream(None))
        assert rc == abi.OK, engine.lib.nexg_ctx_last_error(engine.ctx)
        out = torch.full((total + 4096,), FILL, dtype=torch.uint8, device="cuda")
        t_off = torch.full((k + 3,), -1, dtype=torch.int64, device="cuda")
        t_len = torch.full((k + 2,), -1, dtype=torch.int32, device="cuda")
        t_src = torch.full((k + 2,), -1, dtype=torch.int32, device="cuda")
        rc = engine.lib.nexg_reasm_frames(engine.ctx, ctypes.byref(fr), align, P(d_rows), P(first), P(nbytes), k, P(t_off),
                                          P(t_len), P(t_src), P(out), total, engine._stream(None))
        assert rc == abi.OK, engine.lib.nexg_ctx_last_error(engine.ctx)
        torch.cuda.synchronize()
        hf, hb, r = first.cpu().numpy(), nbytes.cpu().numpy(), d_rows.cpu().numpy()
        assert hf[n] == k and (hf[n + 1:] == -1).all() and hb[n] == total and (hb[n + 1:] == -1).all()
        assert (r[n * 16:] == FILL).all() and (r[: n * 16].view(abi.REASM_DTYPE) == rows).all()
        assert (ws.cpu().numpy()[ws_bytes:] == FILL).all()
        got = out.cpu().numpy()
        assert (got[total:] == FILL).all() and (got[:total] == buf).all()
        assert (t_off.cpu().numpy()[: k + 1] == offs).all() and (t_off.cpu().numpy()[k + 1:] == -1).all()
        assert (t_len.cpu().numpy()[:k] == [len(p) for p in out_frames]).all() and (t_len.cpu().numpy()[k:] == -1).all()
        assert (t_src.cpu().numpy()[:k].view(np.uint32) == src).all() and (t_src.cpu().numpy()[k:] == -1).all()
        runs.append((hf, hb, r, got))
    for a, b in zip(*runs):
        assert (a == b).all()


def test_the_collision_rows(engine):
    frames = list(next(fs for name, _, fs in rf.cases() if name == "collision"))
    want = want_of(frames, 1)
    assert int((want[2]["flags"] == abi.REASM_COLLISION).sum()) == 6 and len(want[0]) == 1
    check(engine, "collision", FrameBatch.from_frames(frames), want, 1)
    # what the host does with the held frames: reassemble_host resolves them exactly
    out, src, rows, collided = reassemble_host(frames)
    assert len(out) == 3 and (collided == (want[2]["flags"] == abi.REASM_COLLISION)).all()


def shuffled(engine, batch, seed):
    """`batch` (packed) with its frames in a seeded random order: a table over the same data, gathered dense."""
    import torch
    perm = np.random.default_rng(seed).permutation(batch.count)
    offs = batch.offsets.cpu().numpy()
    at = torch.from_numpy(perm).cuda()
    table = FrameBatch(data=batch.data, count=batch.count, offsets=batch.offsets[:-1][at],
                       lengths=torch.from_numpy((offs[1:] - offs[:-1]).astype(np.int32)).cuda()[at])
    return engine.gather(table), perm


@pytest.mark.parametrize("ignore_df", (False, True), ids=("df honoured", "df ignored"))
def test_fragment_shuffle_reassemble_on_the_imix_batch(engine, ignore_df):
    """Engine.fragment of the generator's IMIX batch (N = 4096, mtu 576), its
    pieces in a random order, reassembled: every frame the fragment pass gave
    pieces for comes back byte for byte. With DF honoured (ignore_df off)
    nothing is split: every IPv4 frame of the mix over 576 bytes has DF set and
    gives no output, like the IPv6 ones, and the rest passes through both
    ways. Under IGNORE_DF those IPv4 frames leave as three pieces each and come
    back whole, DF cleared as the pieces carry it."""
    import torch
    n = 4096
    b = engine.gen_batch(abi.WL_IMIX, n)
    pieces, p_src, p_rows = engine.fragment(b, 576, ignore_df=ignore_df)
    mixed, perm = shuffled(engine, pieces, 3)
    out, src, rows, (hidx, held) = Reassembler(engine).run(mixed)
    torch.cuda.synchronize()
    frows = helpers.to_host(p_rows, abi.FRAGGED_DTYPE, n)
    n_split, n_big = int((frows["kind"] == abi.FRAG_SPLIT).sum()), int((frows["kind"] == abi.FRAG_TOO_BIG).sum())
    assert (n_split > 100 and n_big > 100 and pieces.count == n - n_big + 2 * n_split) if ignore_df else (n_split == 0 and n_big > 200)
    keep = np.flatnonzero(np.isin(frows["kind"], (abi.FRAG_PASS, abi.FRAG_SPLIT)))
    assert out.count == len(keep) and held.count == 0
    # the input frame of each output: the piece its head or pass-through was, through both indices
    origin = p_src.cpu().numpy().view(np.uint32)[perm[src.cpu().numpy().view(np.uint32)]]
    order = np.argsort(origin, kind="stable")
    assert (origin[order] == keep).all()
    data, offs = out.data.cpu().numpy(), out.offsets.cpu().numpy()
    raw, roffs = b.data.cpu().numpy(), (b.offsets.cpu().numpy() if b.offsets is not None else np.arange(n + 1) * b.stride)
    rlen = b.lengths.cpu().numpy() if b.lengths is not None else roffs[1:] - roffs[:-1]
    for f, i in zip(order, keep):
        frame = raw[roffs[i]:roffs[i] + rlen[i]].tobytes()
        if frows["kind"][i] == abi.FRAG_SPLIT:
            frame = ff.datagram(frame, clear_df=True)
        assert data[offs[f]:offs[f + 1]].tobytes() == frame, i
    # and it is what the host says of the same table
    md, mo = mixed.data.cpu().numpy(), mixed.offsets.cpu().numpy()
    want = want_of([md[mo[i]:mo[i + 1]].tobytes() for i in range(mixed.count)], 1)
    assert (helpers.to_host(rows, abi.REASM_DTYPE, mixed.count) == want[2]).all() and (data == want[3]).all()


@functools.lru_cache(maxsize=None)
def vteps():
    return TunnelSet([Tunnel.vxlan(vni=5000 + t, src="10.0.0.1", dst=f"10.0.1.{t + 1}", eth_dst="02:00:00:00:00:02",
                                   eth_src="02:00:00:00:00:01", src_port=49152, udp_csum=True, ip_id=0x4200 + t)
                      for t in range(16)])


def test_encap_fragment_shuffle_reassemble_parse_decap(engine, oracle):
    """A tunnel endpoint's way out and the peer's way back. The outer header's
    identification is the tunnel's, so each of the 16 tunnels carries one
    frame that has to be split; the others fit the MTU."""
    import torch
    big = [f for f in (oracle.gen_frame(abi.WL_IMIX, i) for i in range(400)) if len(f) >= 1500][:16]
    little = [f for f in (oracle.gen_frame(abi.WL_IMIX, i) for i in range(400)) if len(f) < 600][:48]
    assert len(big) == 16 and len(little) == 48
    inner = big + little
    index = torch.from_numpy((np.arange(len(inner)) % 16).astype(np.uint8)).cuda()
    outer, _ = engine.encap(FrameBatch.from_packed(inner, pad_to=1), vteps(), index)
    pieces, p_src, p_rows = engine.fragment(outer, 1500)
    assert pieces.count == len(inner) + 16
    mixed, perm = shuffled(engine, pieces, 9)
    back, src, rows, (hidx, held) = Reassembler(engine).run(mixed)
    torch.cuda.synchronize()
    assert back.count == len(inner) and held.count == 0
    origin = p_src.cpu().numpy().view(np.uint32)[perm[src.cpu().numpy().view(np.uint32)]]
    rec = engine.parse(back, out_kind=abi.OUT_RECORD)
    flags = helpers.to_host(rec, abi.RECORD_DTYPE, back.count)["flags"]
    assert ((flags & abi.C_IP_OK) != 0).all() and ((flags & abi.C_L4_OK) != 0).all()
    tun, tab = engine.decap(back, rec)
    th = helpers.to_host(tun, abi.TUNNEL_DTYPE, back.count)
    assert (th["kind"] == abi.TUN_VXLAN).all() and (th["status"] == 0).all() and (th["id"] == 5000 + origin % 16).all()
    d2, o2, l2 = back.data.cpu().numpy(), tab.offsets.cpu().numpy(), tab.lengths.cpu().numpy()
    for f, i in enumerate(origin):
        assert d2[o2[f]:o2[f] + l2[f]].tobytes() == inner[i], (f, i)


def test_gather_rows_carries_a_per_frame_row_through(engine):
    import torch
    frames = list(corpus_table()[:3000])
    want = want_of(frames, 1)
    out, d_src, _, _ = Reassembler(engine).run(FrameBatch.from_frames(frames, pad_to=4))
    rule = (np.arange(len(frames), dtype=np.uint32) * 2654435761 + 17).astype(np.uint32)
    got = engine.gather_rows(torch.from_numpy(rule.view(np.int32)).cuda(), 4, d_src)
    torch.cuda.synchronize()
    assert 0 < out.count < len(frames)
    assert (helpers.to_host(got, np.uint32, out.count) == rule[want[1]]).all()


def model_push(state, frames, epoch, min_epoch, max_bytes):
    """Reassembler.push restated with lists: state is [(frame, epoch)]. Returns (outputs, new state, dropped)."""
    whole = [f for f, _ in state] + list(frames)
    eps = [e for _, e in state] + [epoch] * len(frames)
    out, src, rows, _ = reassemble_host(whole, exact=False)
    held = [(whole[i], eps[i]) for i in np.flatnonzero(rows["kind"] == abi.REASM_HELD) if eps[i] >= min_epoch]
    dropped = 0
    while max_bytes is not None and held and sum(len(f) for f, _ in held) > max_bytes:
        oldest = min(e for _, e in held)
        dropped += sum(e == oldest for _, e in held)
        held = [(f, e) for f, e in held if e != oldest]
    return out, held, dropped


def state_of(rs):
    if rs.held_count == 0:
        return []
    d, o = rs._held.data.cpu().numpy(), rs._held.offsets.cpu().numpy()
    e = rs._epochs.cpu().numpy().view(np.uint32)
    return [(d[o[i]:o[i + 1]].tobytes(), int(e[i])) for i in range(rs.held_count)]


def test_push_over_three_batches_with_an_epoch_timeout(engine):
    import torch
    a = rf.train(ff.ipv4(3000, seed=21), 576, 0x6001)   # six pieces over three batches
    b = rf.train(ff.ipv4(1500, seed=22), 576, 0x6002)   # its last piece never comes: times out
    c = rf.train(ff.ipv4(1200, seed=23), 576, 0x6003)   # whole inside batch 2
    d = rf.train(ff.ipv4(2000, seed=24), 576, 0x6004)   # pushed out by max_held_bytes
    whole = ff.ipv4(100, seed=25)
    batches = [([a[4], b[0], whole, a[0]], 1, 0), ([c[1], a[2], a[5], c[0], c[2], b[1]], 2, 0), ([a[1], whole, a[3]], 3, 0),
               ([whole], 4, 2), ([d[0], d[1]], 5, 0), ([b[0]], 6, 0)]
    rs = Reassembler(engine, max_held_bytes=1300)
    state, dropped = [], 0
    for frames, epoch, min_epoch in batches:
        want_out, state, gone = model_push(state, frames, epoch, min_epoch, 1300 if epoch >= 5 else None)
        rs.max_held_bytes = 1300 if epoch >= 5 else None
        dropped += gone
        out, src, rows, _ = rs.push(FrameBatch.from_frames(frames), epoch, min_epoch)
        torch.cuda.synchronize()
        data, offs = out.data.cpu().numpy(), out.offsets.cpu().numpy()
        assert [data[offs[f]:offs[f + 1]].tobytes() for f in range(out.count)] == want_out, epoch
        assert state_of(rs) == state, epoch
        assert rs.held_count == len(state) and rs.held_bytes == sum(len(f) for f, _ in state) and rs.dropped == dropped, epoch
        if epoch == 3:
            assert rf.retag(ff.ipv4(3000, seed=21), 0x6001) in want_out and [e for _, e in state] == [1, 2]
        if epoch == 4:
            assert [e for _, e in state] == [2]  # b[0] of epoch 1 timed out
        if epoch == 5:
            assert dropped == 1 and [e for _, e in state] == [5, 5]
    with pytest.raises(ValueError):
        rs.run(FrameBatch.from_frames([whole]), align=3)
    with pytest.raises(ValueError):
        rs.push(FrameBatch.from_frames([whole]), -1)
