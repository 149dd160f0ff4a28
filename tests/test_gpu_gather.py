"""GPU: the gather of selected frames and rows (nexg_gather_plan,
nexg_gather_frames, nexg_gather_rows).

out_offsets, out_len and every output byte, pads included, must equal
nex_amd.select.gather_host exactly. Shapes: every length at which the copy
kernel changes path (frames shorter than a 16-B chunk, chunk-sized, one more,
jumbo), in runs and interleaved; sources at every byte phase modulo 16; every
alignment; an output capacity that cuts a frame; frames with a bad extent;
a source ending on the data tensor's last byte; the counts around a wave, a
tile and the scan's 256-tile carry."""
import ctypes

import numpy as np
import pytest

from nex_amd import abi
from nex_amd import select as S
from nex_amd.engine import FrameBatch
from nex_amd.frame import ParseMode, ParseOption
from tests import helpers
from tests import select_frames as sf

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 3, 4, 15, 16, 17, 31, 32, 33, 60, 64, 65, 1514, 65535]
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
ALIGNS = (1, 4, 8, 16)
VLAN = ParseOption(unwrap_vlan=True)


def frames_of(lengths, seed=1):
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(1, 256, n, dtype=np.uint8)) for n in lengths]  # no zero byte: pads stand out


def table_batch(data, offs, lens, hints=0):
    """offsets + lengths batch over a host byte array."""
    import torch
    return FrameBatch(data=torch.from_numpy(np.ascontiguousarray(data)).cuda(), count=len(offs),
                      offsets=torch.from_numpy(np.asarray(offs, np.int64)).cuda(),
                      lengths=torch.from_numpy(np.asarray(lens, np.uint32).view(np.int32)).cuda(), hints=hints)


def host_table(batch):
    if batch.offsets is None:
        off = np.arange(batch.count, dtype=np.int64) * batch.stride
    else:
        off = batch.host_offsets()[: batch.count]
    return off, batch.frame_lengths()


def check_gather(engine, name, batch, align):
    import torch
    off, ln = host_table(batch)
    want_off, want_len, want = S.gather_host(batch.data.cpu().numpy(), off, ln, align)
    out = engine.gather(batch, align)
    torch.cuda.synchronize()
    n = batch.count
    assert out.count == n and out.data.numel() == len(want), (name, out.data.numel(), len(want))
    assert (out.offsets.cpu().numpy().astype(np.uint64) == want_off).all(), name
    if align == 1:
        assert out.lengths is None
    else:
        assert (out.lengths.cpu().numpy().view(np.uint32) == want_len).all(), name
    got = out.data.cpu().numpy()
    if not (got == want).all():
        bad = int(np.nonzero(got != want)[0][0])
        k = int(np.searchsorted(want_off, bad, side="right")) - 1
        raise AssertionError(f"{name}: byte {bad} (frame {k}, at {bad - int(want_off[k])} of {int(want_len[k])}) "
                             f"is {got[bad]}, want {want[bad]}")
    return out


def shifted_packed(frames, shift):
    """Packed batch whose first frame starts `shift` bytes into the data (the
    data pointer itself stays aligned), ending on the data tensor's last byte."""
    import torch
    offs = np.zeros(len(frames) + 1, np.int64)
    offs[1:] = np.cumsum([len(f) for f in frames])
    offs += shift
    buf = np.full(max(int(offs[-1]), 16), 0xEE, np.uint8)  # (a batch of empty frames still needs a data pointer)
    buf[shift:int(offs[-1])] = np.frombuffer(b"".join(frames), np.uint8)
    return FrameBatch(data=torch.from_numpy(buf).cuda(), count=len(frames), offsets=torch.from_numpy(offs).cuda())


@pytest.mark.parametrize("align", ALIGNS)
def test_lengths_in_runs_and_interleaved(engine, align):
    runs = [n for n in LENGTHS for _ in range(3)]
    inter = LENGTHS + LENGTHS[::-1] + [0, 0, 1, 0, 16, 0, 0, 17, 0]
    for name, lens in (("runs", runs), ("interleaved", inter), ("only empty", [0] * 70), ("only tiny", [1, 2, 3] * 100)):
        fr = frames_of(lens)
        check_gather(engine, f"{name} align {align} packed", shifted_packed(fr, 0), align)
        check_gather(engine, f"{name} align {align} offsets+lengths", FrameBatch.from_frames(fr, pad_to=4), align)


@pytest.mark.parametrize("shift", range(16))
def test_every_source_phase(engine, shift):
    lens = [n for n in LENGTHS if n < 2000] + [16, 16, 48, 5, 32, 100, 7, 64]
    fr = frames_of(lens, seed=shift)
    batch = shifted_packed(fr, shift)
    for align in ALIGNS:
        check_gather(engine, f"shift {shift} align {align}", batch, align)


@pytest.mark.parametrize("count", COUNTS)
def test_counts(engine, count):
    lens = [LENGTHS[i % 13] if i % 97 else 1514 for i in range(count)]
    fr = frames_of(lens, seed=count)
    for align in (1, 16):
        check_gather(engine, f"n={count} align {align}", shifted_packed(fr, 3), align)


def test_65793_frames_of_64_bytes(engine):
    batch = engine.gen_batch(abi.WL_UDP64, 65793)
    assert batch.stride == 64 and batch.offsets is None
    for align in (1, 16):
        out = check_gather(engine, f"65793 x 64 align {align}", batch, align)
        assert out.data.numel() == 65793 * 64
    # and from a table that is not the identity: every third frame, twice
    import torch
    off = (torch.arange(65793, device="cuda", dtype=torch.int64) * 3 % 65793) * 64
    ln = torch.full((65793,), 61, dtype=torch.int32, device="cuda")
    sel = FrameBatch(data=batch.data, count=65793, offsets=off, lengths=ln)
    for align in (1, 4):
        check_gather(engine, f"65793 x 61 align {align}", sel, align)


def _raw_frames(engine, sel, offs, out, cap):
    fr = sel.to_c()
    return engine.lib.nexg_gather_frames(engine.ctx, ctypes.byref(fr), ctypes.c_void_p(offs.data_ptr()),
                                         ctypes.c_void_p(out.data_ptr()), cap, engine._stream(None))


@pytest.mark.parametrize("align", (1, 16))
def test_out_cap_bounds_every_store(engine, align):
    import torch
    lens = [60, 0, 17, 1514, 3, 64, 65, 16, 31] * 40
    fr = frames_of(lens, seed=9)
    batch = shifted_packed(fr, 5)
    off, ln = host_table(batch)
    want_off, want_len, want = S.gather_host(batch.data.cpu().numpy(), off, ln, align)
    total = len(want)
    plan = engine.gather(batch, align)  # the planned offsets
    mid = int(want_off[200]) + 7           # inside a frame
    assert want_off[200] + want_len[200] > mid
    edge = int(want_off[123])              # on a frame boundary
    for cap in (0, 1, mid, edge, 16 * (edge // 16), total - 1, total):
        out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        assert _raw_frames(engine, batch, plan.offsets, out, cap) == abi.OK
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[cap:] == 0xA5).all(), (align, cap, int(np.nonzero(got[cap:] != 0xA5)[0][0]) + cap)
        assert (got[:cap] == want[:cap]).all(), (align, cap)
    # out_offsets is caller memory: garbage in it moves no store to or past out_cap
    rng = np.random.default_rng(3)
    junk = plan.offsets.cpu().numpy().copy()
    hit = rng.integers(0, len(junk), 60)
    junk[hit] = rng.integers(0, 1 << 62, 60)
    junk[7], junk[300] = (1 << 63) - 1, 0
    jt = torch.from_numpy(junk).cuda()
    out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    assert _raw_frames(engine, batch, jt, out, total) == abi.OK
    torch.cuda.synchronize()
    assert (out.cpu().numpy()[total:] == 0xA5).all()


def test_bad_frames_copy_as_length_0(engine):
    import torch
    data = np.frombuffer(b"".join(frames_of([4000], seed=4)), np.uint8).copy()
    offs = [0, 3990, 3999, 4000, 4001, 100, (1 << 40), 50, 0]
    lens = [10, 10, 2, 0, 0, 70000, 4, 65536, 4000]
    want_copied = [10, 10, 0, 0, 0, 0, 0, 0, 4000]
    batch = table_batch(data, offs, lens)
    for align in ALIGNS:
        out = check_gather(engine, f"bad extents align {align}", batch, align)
        torch.cuda.synchronize()
        o = out.offsets.cpu().numpy()
        pad = lambda n: (n + align - 1) // align * align  # noqa: E731
        assert np.diff(o).tolist() == [pad(n) for n in want_copied]


def test_source_ending_on_the_last_byte(engine):
    for last in (1, 15, 16, 17, 64, 1514):
        fr = frames_of([33, 64, last], seed=last)
        batch = shifted_packed(fr, 0)
        assert batch.data.numel() == 33 + 64 + last
        for align in ALIGNS:
            out = check_gather(engine, f"last {last} align {align}", batch, align)
            o = out.offsets.cpu().numpy()
            assert out.data.cpu().numpy()[int(o[2]): int(o[2]) + last].tobytes() == fr[2]


def test_round_trip_through_select_and_parse(engine, oracle):
    """The parse of the gathered batch equals records[index]."""
    c = sf.corpus()
    which = np.arange(700) % len(c)
    frames = [c[i].frame for i in which]
    recs_host = oracle.parse_frames([x.frame for x in c], sf.PARSE_FLAGS)[which]
    batch = FrameBatch.from_packed(frames, pad_to=1, shift=4)
    recs = engine.parse(batch, VLAN, ParseMode.Strict, out_kind=abi.OUT_RECORD)
    for name in ("issue examples", "inverted", "match all"):
        idx, sel = engine.select(batch, recs, sf.FILTERS[name])
        pick = idx.cpu().numpy().view(np.uint32)
        assert len(pick) > 0
        for align in (1, 8):
            dense = check_gather(engine, f"round trip {name} align {align}", sel, align)
            got = engine.parse_to_numpy(dense, VLAN, ParseMode.Strict, out_kind=abi.OUT_RECORD)
            helpers.records_equal(got, recs_host[pick], [frames[i] for i in pick], f"parse(gather) {name} {align}")


@pytest.mark.parametrize("row_bytes", abi.GATHER_ROW_BYTES)
def test_gather_rows(engine, row_bytes):
    import torch
    rng = np.random.default_rng(row_bytes)
    nrows = 1000
    rows = rng.integers(1, 256, (nrows, row_bytes), dtype=np.uint8)
    index = np.concatenate([rng.integers(0, nrows, 700), [nrows, nrows + 1, 0xFFFFFFFF, 0, nrows - 1]]).astype(np.uint32)
    rng.shuffle(index)
    dev_rows = torch.from_numpy(rows.reshape(-1)).cuda()
    dev_idx = torch.from_numpy(index.view(np.int32)).cuda()
    got = engine.gather_rows(dev_rows, row_bytes, dev_idx).cpu().numpy().reshape(-1, row_bytes)
    want = np.where((index < nrows)[:, None], rows[np.minimum(index, nrows - 1)], 0)
    assert (got == want).all()
    assert (index >= nrows).sum() == 3 and not got[index >= nrows].any()
    # n == 0 launches nothing and returns an empty tensor
    assert engine.gather_rows(dev_rows, row_bytes, dev_idx[:0]).numel() == 0
    for n in (1, 63, 64, 65, 255, 256, 257):
        g = engine.gather_rows(dev_rows, row_bytes, dev_idx[:n]).cpu().numpy().reshape(-1, row_bytes)
        assert (g == want[:n]).all(), n


def test_gather_argument_errors(engine):
    import torch
    fr = frames_of([60, 64, 65])
    batch = shifted_packed(fr, 0)
    with pytest.raises(ValueError):
        engine.gather(batch, 2)
    with pytest.raises(ValueError):
        engine.gather_rows(batch.data, 12, torch.zeros(1, dtype=torch.int32, device="cuda"))
    lib, ctx, s = engine.lib, engine.ctx, engine._stream(None)
    c = batch.to_c()
    offs = torch.zeros(8, dtype=torch.int64, device="cuda")
    wsb = abi.gather_plan_workspace(3)
    ws = torch.zeros(wsb // 8 + 1, dtype=torch.int64, device="cuda")
    P = lambda t, d=0: ctypes.c_void_p(t.data_ptr() + d)  # noqa: E731
    assert lib.nexg_gather_plan(ctx, ctypes.byref(c), 1, P(offs), None, P(ws), wsb, s) == abi.OK
    for align in (0, 2, 3, 32):
        assert lib.nexg_gather_plan(ctx, ctypes.byref(c), align, P(offs), None, P(ws), wsb, s) == abi.EINVAL
    assert lib.nexg_gather_plan(ctx, ctypes.byref(c), 1, None, None, P(ws), wsb, s) == abi.EINVAL
    assert lib.nexg_gather_plan(ctx, ctypes.byref(c), 1, P(offs), None, None, wsb, s) == abi.EINVAL
    assert lib.nexg_gather_plan(ctx, ctypes.byref(c), 1, P(offs), None, P(ws), wsb - 1, s) == abi.EINVAL
    assert lib.nexg_gather_plan(ctx, ctypes.byref(c), 1, P(offs, 4), None, P(ws), wsb, s) == abi.EINVAL
    out = torch.zeros(256, dtype=torch.uint8, device="cuda")
    assert lib.nexg_gather_frames(ctx, ctypes.byref(c), P(offs), P(out, 8), 200, s) == abi.EINVAL
    assert lib.nexg_gather_frames(ctx, ctypes.byref(c), None, P(out), 200, s) == abi.EINVAL
    assert lib.nexg_gather_frames(ctx, ctypes.byref(c), P(offs), None, 200, s) == abi.EINVAL
    idx = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert lib.nexg_gather_rows(ctx, P(out), 12, 4, P(idx), 4, P(out, 128), s) == abi.EINVAL
    assert lib.nexg_gather_rows(ctx, P(out, 8), 16, 4, P(idx), 4, P(out, 128), s) == abi.EINVAL
    assert lib.nexg_gather_rows(ctx, P(out), 16, 4, None, 4, P(out, 128), s) == abi.EINVAL
    assert lib.nexg_gather_rows(ctx, P(out), 16, 4, P(idx), 4, P(out, 128), s) == abi.OK
    torch.cuda.synchronize()
    # an empty table plans a total of 0
    empty = FrameBatch.from_packed([], pad_to=1)
    assert engine.gather(empty, 16).count == 0
