"""GPU: nexg_recompute_checksums_batch and nexg_checksum_batch over the sweep
of tests/fixup_sweep.py: every table layout, frames at every 16-B phase and
both address parities, payloads up to the 65535-B ceiling, raw-IP frames at
odd ip_offsets, the planted fold edges; the whole data tensor, its guards and
the report are compared with the oracle's, bit for bit.
tests/test_fixup_sweep.py checks the corpus, the references and the comparer
on the CPU; tests/test_gpu_fixup.py holds the reference's own relations."""
import ctypes

import numpy as np
import pytest

from nex_amd import abi
from nex_amd.engine import FrameBatch, _frames, _ptr
from nex_amd.frame import ParseOption
from tests import fixup_sweep as fs
from tests import helpers

pytestmark = pytest.mark.gpu

GB, GA, FILL = fs.GUARD_BEFORE, fs.GUARD_AFTER, fs.GUARD_FILL


@pytest.fixture(scope="module")
def corpus(oracle):
    fs.check_corpus()
    return fs.corpus()


def extents(batch):
    """(offsets, lengths) of every frame in batch.data, on the host."""
    lens = batch.frame_lengths()
    if batch.offsets is None:
        return np.arange(batch.count, dtype=np.int64) * batch.stride, lens
    return batch.host_offsets()[: batch.count], lens


def guarded(batch, host_data):
    """A fresh copy of `host_data` (the batch's unfixed bytes) between GUARD_FILL
    guards, at the 16-B phase of the batch's own data pointer, under the
    batch's tables: (whole tensor, offset of data in it, batch)."""
    import torch
    n = len(host_data)
    lo = GB + (batch.data.data_ptr() % 16 if batch.count else 0)
    big = torch.full((lo + n + GA,), FILL, dtype=torch.uint8, device="cuda")
    assert big.data_ptr() % 16 == 0
    big[lo:lo + n] = torch.from_numpy(np.ascontiguousarray(host_data))
    return big, lo, FrameBatch(data=big[lo:lo + n], count=batch.count, stride=batch.stride, offsets=batch.offsets,
                               lengths=batch.lengths, hints=batch.hints)


def fix(engine, batch, which, mode, report=True):
    """(whole host buffer, report rows or None) after the fix-up of a guarded batch."""
    import torch
    big, lo, gb = batch
    out = engine.recompute_checksums(gb, which, ParseOption(*mode), report=report)
    torch.cuda.synchronize()
    rep = None if out is None else out.cpu().numpy()[: gb.count * 8].view(abi.FIXUP_DTYPE)
    return big.cpu().numpy(), rep


def sweep_layout(engine, name, batch, keep, fixed, rep, which, mode):
    host = batch.data.cpu().numpy().copy() if batch.count else np.zeros(batch.data.numel(), np.uint8)
    offs, lens = extents(batch)
    keep = np.arange(len(fixed)) if keep is None else keep
    want = fs.expected_buffer(host, offs, lens, [fixed[i] for i in keep])
    g = guarded(batch, host)
    buf, got = fix(engine, g, which, mode)
    fs.compare(buf, want, offs, lens, got, rep[keep], lo=g[1], what=f"{name}, which {which}, mode {mode}")
    g = guarded(batch, host)
    buf, _ = fix(engine, g, which, mode, report=False)
    fs.compare(buf, want, offs, lens, lo=g[1], what=f"{name}, which {which}, mode {mode}, no report")
    return g[2], offs, got


@pytest.mark.parametrize("which", fs.WHICH)
@pytest.mark.parametrize("mode", [(False, 0), (True, 14)], ids=["eth", "from_ip14"])
def test_fixup_sweep(engine, oracle, corpus, which, mode):
    frames = list(corpus.frames)
    fixed, rep = fs.oracle_fixed(corpus.frames, which, *mode)
    lays = helpers.layouts(frames, strided_below=4096)
    assert len(lays) == 6
    for name, b, keep in lays:
        # the fix-up never runs on b.data itself (with_offsets32() shares it with its parent):
        # every run gets a fresh guarded copy of the unfixed bytes under b's tables
        sweep_layout(engine, name, b, keep, fixed, rep, which, mode)


def test_fixup_phases(engine, oracle, corpus):
    """The structured frames of at most 4 KiB and three long ones, packed with
    the first frame at each shift 0..15: both address parities and all 16
    phases of the L4 range's start occur among the frames fixed at L4."""
    import torch
    idx = [i for i in corpus.structured if len(corpus.frames[i]) <= 4096]
    longs = [i for i in corpus.structured if len(corpus.frames[i]) > 16384]
    idx += [longs[0], longs[len(longs) // 2], next(i for i in longs if len(corpus.frames[i]) == fs.MAX_FRAME)]
    frames = tuple(corpus.frames[i] for i in idx)
    assert sum(len(f) > 16384 for f in frames) == 3
    fixed, rep = fs.oracle_fixed(frames, fs.BOTH, False, 0)
    l4 = (rep["done"] & abi.FIX_L4) != 0
    phases = set()
    for shift in range(16):
        data, offs = fs.pack(frames, shift=shift)
        b = FrameBatch(data=torch.from_numpy(data).cuda(), count=len(frames), offsets=torch.from_numpy(offs).cuda())
        gb, o, _ = sweep_layout(engine, f"packed from byte {shift}", b, None, fixed, rep, fs.BOTH, (False, 0))
        phases |= set(((gb.data.data_ptr() + o[l4] + rep["l4_off"][l4]) % 16).tolist())
    assert phases == set(range(16))


@pytest.mark.parametrize("k", fs.RAW_OFFSETS)
def test_fixup_raw_ip_at_odd_offsets(engine, oracle, corpus, k):
    frames = fs.raw_ip(k)
    fixed, rep = fs.oracle_fixed(frames, fs.BOTH, True, k)
    assert ((rep["done"] & abi.FIX_L4) != 0).sum() >= 200
    for name, b in (("packed from byte 1", helpers.packed_from_byte_1(list(frames))),
                    ("offsets + lengths", FrameBatch.from_frames(list(frames), pad_to=4))):
        sweep_layout(engine, f"raw_ip({k}) {name}", b, None, fixed, rep, fs.BOTH, (True, k))


@pytest.mark.parametrize("count", [0, 1, 255, 256, 257])
def test_fixup_counts(engine, oracle, corpus, count):
    small = [f for f in corpus.frames if len(f) <= 4096]
    frames = tuple(small[i] for i in np.linspace(0, len(small) - 1, count).astype(int))  # spread over the corpus
    assert len(frames) == count
    fixed, rep = fs.oracle_fixed(frames, fs.BOTH, False, 0)
    sweep_layout(engine, f"{count} frames", helpers.packed_from_byte_1(list(frames)), None, fixed, rep, fs.BOTH,
                 (False, 0))


def test_fixup_idempotent_and_verifies(engine, oracle, corpus):
    """A second fix-up of the fixed batch changes no byte and returns the same
    report; the written values are the stored checksums of a parse of the fixed
    batch, and where the packet API's checksum of the unfixed frame (what the
    parse verifies against) equals the value written, the parse verifies it."""
    frames = list(corpus.frames)
    fixed, rep = fs.oracle_fixed(corpus.frames, fs.BOTH, False, 0)
    b = helpers.packed_from_byte_1(frames)
    before = engine.parse_to_numpy(b, out_kind=abi.OUT_RECORD)
    g = guarded(b, b.data.cpu().numpy().copy())
    buf1, rep1 = fix(engine, g, fs.BOTH, (False, 0))
    buf2, rep2 = fix(engine, g, fs.BOTH, (False, 0))
    assert (buf1 == buf2).all() and rep1.tobytes() == rep2.tobytes() == rep.tobytes()
    after = engine.parse_to_numpy(g[2], out_kind=abi.OUT_RECORD)
    ip = ((rep["done"] & abi.FIX_IP) != 0) & ((before["flags"] & abi.C_IP_CHECKED) != 0)
    l4 = ((rep["done"] & abi.FIX_L4) != 0) & ((before["flags"] & abi.C_L4_CHECKED) != 0) & \
        (before["l4_off"] == rep["l4_off"])
    assert (after["ip_csum"][ip] == rep["ip_csum"][ip]).all() and (after["l4_csum"][l4] == rep["l4_csum"][l4]).all()
    ip &= before["ip_csum_calc"] == rep["ip_csum"]
    l4 &= before["l4_csum_calc"] == rep["l4_csum"]
    # the oracle's parse of the same corpus puts 803 / 1964 frames here: the frames whose lengths are exact
    assert ip.sum() >= 300 and l4.sum() >= 300, (ip.sum(), l4.sum())
    assert ((after["flags"][ip] & abi.C_IP_OK) != 0).all() and ((after["flags"][l4] & abi.C_L4_OK) != 0).all()


def test_fixup_refuses_bad_extents(engine, oracle, corpus):
    """Every way frame_extent refuses an entry: the report row is zero and no
    byte changes. Every entry lies inside the tensor the test owns."""
    import torch
    done = fs.oracle_fixed(corpus.frames, fs.BOTH, False, 0)[1]["done"]
    f = next(x for x, d in zip(corpus.frames, done) if 1000 < len(x) < 2000 and d == fs.BOTH)
    n = 65536 + 70000 + 2048
    data = np.random.default_rng(5).integers(0, 256, n, dtype=np.uint8)
    at = 65536 + 70000
    data[at:at + len(f)] = np.frombuffer(f, np.uint8)
    offs = np.array([0, 65536, n, n, n + 1, n - 4, at], np.int64)
    lens = np.array([65536, 70000, 0, 1, 0, 5, len(f)], np.int32)
    assert GA >= 2
    fixed, rep = fs.oracle_fixed((f,), fs.BOTH, False, 0)
    assert rep[0]["done"] == fs.BOTH
    want = fs.expected_buffer(data, offs[-1:], lens[-1:], fixed)
    b = FrameBatch(data=torch.from_numpy(data).cuda(), count=len(offs), offsets=torch.from_numpy(offs).cuda(),
                   lengths=torch.from_numpy(lens).cuda())
    want_rep = np.zeros(len(offs), abi.FIXUP_DTYPE)
    want_rep[-1] = rep[0]
    for name, batch in (("u64 table", b), ("u32 table", b.with_offsets32())):
        g = guarded(batch, data)
        buf, got = fix(engine, g, fs.BOTH, (False, 0))
        fs.compare(buf, want, offs, lens, got, want_rep, lo=g[1], what=f"refused extents, {name}")


def test_fixup_rejections(engine, corpus):
    import torch
    b = FrameBatch.from_frames(list(corpus.frames[:8]), pad_to=4)
    before = b.data.cpu().numpy().copy()
    opt = abi.ParseOptionC(0, 0)
    rows = torch.zeros(8 * 8 + 16, dtype=torch.uint8, device="cuda")
    assert rows.data_ptr() % 8 == 0

    def call(frames, which, out):
        rc = engine.lib.nexg_recompute_checksums_batch(engine.ctx, frames, ctypes.byref(opt), which, out,
                                                       engine._stream(None))
        return rc, engine.lib.nexg_ctx_last_error(engine.ctx).decode()

    for which in (4, 8, 0x80000000 | fs.BOTH):
        rc, msg = call(_frames(b), which, _ptr(rows))
        assert rc == abi.EINVAL and "invalid fix-up selection" in msg, (which, rc, msg)
    rc, msg = call(_frames(b), fs.BOTH, _ptr(rows[4:]))
    assert rc == abi.EINVAL and "misaligned" in msg, (rc, msg)
    bad = b.to_c()
    bad.offsets, bad.stride = None, 0  # neither a table nor a stride
    rc, msg = call(ctypes.byref(bad), fs.BOTH, _ptr(rows))
    assert rc == abi.EINVAL and "invalid frame batch" in msg, (rc, msg)
    bad = FrameBatch(data=b.data[2:], count=b.count, offsets=b.offsets, lengths=b.lengths).to_c()  # data at 2 mod 4
    rc, msg = call(ctypes.byref(bad), fs.BOTH, _ptr(rows))
    assert rc == abi.EINVAL and "invalid frame batch" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert (b.data.cpu().numpy() == before).all() and not rows.cpu().numpy().any()


def test_checksum_batch_sweep(engine, oracle):
    """checksum_cases() packed at shifts 0, 1, 2, 3 and 15 and as offsets +
    lengths, against oracle.checksum; the output sits inside a guarded int16
    tensor and nothing outside its count entries is written."""
    import torch
    groups = {}
    for c in fs.checksum_cases():
        groups.setdefault(c.skipword, []).append(c)
    for skip, cases in groups.items():
        want = np.array([oracle.checksum(c.data, skip) if c.want is None else c.want for c in cases], np.uint16)
        datas = [c.data for c in cases]
        batches = []
        for shift in (0, 1, 2, 3, 15):
            data, offs = fs.pack(datas, shift=shift)
            batches.append((f"packed from byte {shift}", FrameBatch(
                data=torch.from_numpy(data).cuda(), count=len(datas), offsets=torch.from_numpy(offs).cuda())))
        batches.append(("offsets + lengths", FrameBatch.from_frames(datas, pad_to=4)))
        for name, b in batches:
            big = torch.full((8 + len(datas) + 32,), -23131, dtype=torch.int16, device="cuda")  # 0xA5A5
            out = big[8:8 + len(datas)]
            engine._check(engine.lib.nexg_checksum_batch(engine.ctx, _frames(b), skip, _ptr(out), engine._stream(None)))
            torch.cuda.synchronize()
            host = big.cpu().numpy().view(np.uint16)
            got = host[8:8 + len(datas)]
            bad = np.nonzero(got != want)[0]
            assert not len(bad), (name, skip, [(int(i), len(datas[i]), hex(got[i]), hex(want[i])) for i in bad[:5]])
            assert (host[:8] == 0xA5A5).all() and (host[8 + len(datas):] == 0xA5A5).all(), (name, skip)
