"""GPU: what nexg_fragment_plan and nexg_fragment_frames refuse (include/nexg.h),
each with NEXG_EINVAL and the context's last error set, and nothing launched:
the prefixes, rows, workspace, table and output keep what they held. And the
empty batch, which launches nothing but the totals."""
import ctypes

import numpy as np
import pytest

from nex_amd import abi
from nex_amd.engine import FrameBatch
from nex_amd.fragment import FragOption, fragment_host, plan_host
from tests import fragment_frames as ff

pytestmark = pytest.mark.gpu

N = 300
FILL = 0xA5


def _p(t, step=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + step)


class Calls:
    """A valid plan and a valid fill over 300 frames, and variations of them."""

    def __init__(self, engine):
        import torch
        small = [f for f in ff.frames() if f is not None and len(f) < 2100]
        self.engine = engine
        self.frames = [small[i % len(small)] for i in range(N)]
        self.batch = FrameBatch.from_packed(self.frames, pad_to=1)
        self.option = FragOption(576)
        self.pieces, self.src, self.rows = fragment_host(self.frames, 576)
        self.K = len(self.pieces)
        self.offs = plan_host([len(p) for p in self.pieces], 1)
        self.total = int(self.offs[-1])
        u8 = lambda n: torch.full((n,), FILL, dtype=torch.uint8, device="cuda")  # noqa: E731
        self.d_first, self.d_bytes, self.d_rows = u8((N + 3) * 4), u8((N + 2) * 8), u8((N + 2) * 16)
        self.ws_bytes = abi.fragment_plan_workspace(N)
        self.d_ws = u8(self.ws_bytes + 16)
        first = np.concatenate([self.rows["first"], [self.K]]).astype(np.uint32)
        self.d_good_first = torch.from_numpy(first.view(np.int32)).cuda()
        self.d_good_bytes = torch.from_numpy(self.offs[first.astype(np.int64)]).cuda()
        self.d_off, self.d_len, self.d_src = u8((self.K + 2) * 8), u8((self.K + 2) * 4), u8((self.K + 2) * 4)
        self.d_out = u8(self.total + 64)

    def _untouched(self, *tensors):
        import torch
        torch.cuda.synchronize()
        return all(bool((t == FILL).all()) for t in tensors)

    def plan(self, **ch):
        a = dict(frames=self.batch.to_c(), option=self.option.to_c(), first=_p(self.d_first), bytes=_p(self.d_bytes),
                 rows=_p(self.d_rows), ws=_p(self.d_ws), ws_bytes=self.ws_bytes)
        a.update(ch)
        for t in (self.d_first, self.d_bytes, self.d_rows, self.d_ws):
            t.fill_(FILL)
        lib, eng = self.engine.lib, self.engine
        ref = lambda v: None if v is None else ctypes.byref(v)  # noqa: E731
        rc = lib.nexg_fragment_plan(eng.ctx, ref(a["frames"]), ref(a["option"]), a["first"], a["bytes"], a["rows"], a["ws"],
                                    a["ws_bytes"], eng._stream(None))
        return rc, lib.nexg_ctx_last_error(eng.ctx).decode(), self._untouched(self.d_first, self.d_bytes, self.d_rows, self.d_ws)

    def fill(self, **ch):
        a = dict(frames=self.batch.to_c(), option=self.option.to_c(), first=_p(self.d_good_first), bytes=_p(self.d_good_bytes),
                 count=self.K, off=_p(self.d_off), len=_p(self.d_len), src=_p(self.d_src), out=_p(self.d_out), cap=self.total)
        a.update(ch)
        for t in (self.d_off, self.d_len, self.d_src, self.d_out):
            t.fill_(FILL)
        lib, eng = self.engine.lib, self.engine
        ref = lambda v: None if v is None else ctypes.byref(v)  # noqa: E731
        rc = lib.nexg_fragment_frames(eng.ctx, ref(a["frames"]), ref(a["option"]), a["first"], a["bytes"], a["count"], a["off"],
                                      a["len"], a["src"], a["out"], a["cap"], eng._stream(None))
        return rc, lib.nexg_ctx_last_error(eng.ctx).decode(), self._untouched(self.d_off, self.d_len, self.d_src, self.d_out)

    def table(self, **kw):
        fr = self.batch.to_c()
        for k, v in kw.items():
            setattr(fr, k, v)
        return fr


@pytest.fixture(scope="module")
def calls(engine):
    return Calls(engine)


def refused(result, text, what):
    rc, got, untouched = result
    assert rc == abi.EINVAL and text in got and untouched, (what, rc, got, untouched)


def test_the_valid_calls_are_accepted(calls):
    K = calls.K
    rc, text, untouched = calls.plan()
    assert rc == abi.OK and not untouched, text
    first = calls.d_first.cpu().numpy()
    assert (first[: (N + 1) * 4].view(np.uint32) == np.concatenate([calls.rows["first"], [K]])).all() and (first[(N + 1) * 4:] == FILL).all()
    nbytes = calls.d_bytes.cpu().numpy()
    assert (nbytes[: (N + 1) * 8].view(np.int64) == calls.d_good_bytes.cpu().numpy()).all() and (nbytes[(N + 1) * 8:] == FILL).all()
    rows = calls.d_rows.cpu().numpy()
    assert (rows[: N * 16].view(abi.FRAGGED_DTYPE) == calls.rows).all() and (rows[N * 16:] == FILL).all()
    assert (calls.d_ws.cpu().numpy()[calls.ws_bytes:] == FILL).all()
    rc, text, untouched = calls.fill()
    assert rc == abi.OK and not untouched, text
    out = calls.d_out.cpu().numpy()
    assert out[: calls.total].tobytes() == b"".join(calls.pieces) and (out[calls.total:] == FILL).all()
    off, ln, src = calls.d_off.cpu().numpy(), calls.d_len.cpu().numpy(), calls.d_src.cpu().numpy()
    assert (off[: (K + 1) * 8].view(np.int64) == calls.offs).all() and (off[(K + 1) * 8:] == FILL).all()
    assert (ln[: K * 4].view(np.uint32) == [len(p) for p in calls.pieces]).all() and (ln[K * 4:] == FILL).all()
    assert (src[: K * 4].view(np.uint32) == calls.src).all() and (src[K * 4:] == FILL).all()
    rc, text, _ = calls.plan(rows=None)  # optional
    assert rc == abi.OK, text


def test_invalid_options_are_refused_by_both(calls):
    bad = {"mtu 67": FragOption(67), "mtu 65536": FragOption(65536), "mtu 0": FragOption(0), "unknown flag": FragOption(576, 2),
           "every flag bit": FragOption(576, 0xFFFFFFFF), "align 0": FragOption(576, 0, 0), "align 2": FragOption(576, 0, 2),
           "align 32": FragOption(576, 0, 32), "reserved": FragOption(576, 0, 1, 1)}
    for name, o in bad.items():
        with pytest.raises(ValueError):
            o.validate()
        refused(calls.plan(option=o.to_c(check=False)), "fragment_plan: ", name)
        refused(calls.fill(option=o.to_c(check=False)), "fragment_frames: ", name)
    refused(calls.plan(option=None), "NULL option", "NULL option")
    refused(calls.fill(option=None), "NULL option", "NULL option")
    for good in (FragOption(68), FragOption(65535, abi.FRAG_IGNORE_DF, 16)):
        rc, text, _ = calls.plan(option=good.to_c())
        assert rc == abi.OK, text


def test_tables(calls):
    for name, fr in {"NULL data": calls.table(data=None), "misaligned data": calls.table(data=calls.batch.data.data_ptr() + 1),
                     "no offsets, no stride": calls.table(offsets=None, stride=0)}.items():
        refused(calls.plan(frames=fr), "invalid frame batch", name)
        refused(calls.fill(frames=fr), "invalid frame batch", name)
    refused(calls.plan(frames=None), "invalid frame batch", "NULL frames")
    refused(calls.fill(frames=None), "invalid frame batch", "NULL frames")
    many = calls.table(count=1 << 32)
    refused(calls.plan(frames=many), "more than 2^32 - 1 frames", "2^32 frames")
    refused(calls.fill(frames=many), "more than 2^32 - 1 frames", "2^32 frames")
    refused(calls.fill(count=1 << 32), "more than 2^32 - 1 output frames", "2^32 output frames")


def test_a_piece_total_past_32_bits_is_reported_by_the_plan(engine):
    """The output frames are numbered with 32 bits and only the device knows
    their total: the plan sums it in 64 bits and writes 2^32 - 1 for 2^32 - 1
    or more. A table whose every entry is the one 65535-byte frame with 60
    header bytes gives 8183 pieces per entry at mtu 68: 524,900 entries pass
    2^32, 524,800 do not. Only the plan runs (it reads four header words per
    entry)."""
    import torch
    big = dict(ff.corpus())["65535 bytes, hl 60"]
    one = FrameBatch.from_frames([big])
    for n, over in ((524_800, False), (524_900, True)):
        assert (n * 8183 >= 0xFFFFFFFF) == over
        batch = FrameBatch(data=one.data, count=n, offsets=one.offsets[:1].repeat(n), lengths=one.lengths[:1].repeat(n))
        first = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        nbytes = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        ws_bytes = abi.fragment_plan_workspace(n)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        fr, oc = batch.to_c(), FragOption(68).to_c()
        rc = engine.lib.nexg_fragment_plan(engine.ctx, ctypes.byref(fr), ctypes.byref(oc), _p(first), _p(nbytes), None, _p(ws),
                                           ws_bytes, engine._stream(None))
        torch.cuda.synchronize()
        assert rc == abi.OK
        total = int(first[n].item()) & 0xFFFFFFFF
        assert total == (abi.FRAG_TOTAL_OVERFLOW if over else n * 8183), (n, total)
        assert int(nbytes[n].item()) == n * (8182 * (74 + 8) + 74 + 5)  # the bytes are summed in 64 bits: never wrapped
        if over:
            with pytest.raises(ValueError):
                engine.fragment(batch, 68)


def test_plan_arguments(calls):
    refused(calls.plan(first=None), "NULL out_first or out_bytes", "NULL out_first")
    refused(calls.plan(bytes=None), "NULL out_first or out_bytes", "NULL out_bytes")
    refused(calls.plan(ws=None), "NULL workspace", "NULL workspace")
    refused(calls.plan(ws_bytes=calls.ws_bytes - 1), "workspace smaller than nexg_fragment_plan_workspace", "small workspace")
    refused(calls.plan(first=_p(calls.d_first, 2)), "misaligned", "out_first + 2")
    refused(calls.plan(bytes=_p(calls.d_bytes, 4)), "misaligned", "out_bytes + 4")
    refused(calls.plan(rows=_p(calls.d_rows, 8)), "misaligned", "rows + 8")
    refused(calls.plan(ws=_p(calls.d_ws, 4)), "misaligned", "workspace + 4")


def test_fill_arguments(calls):
    refused(calls.fill(first=None), "NULL out_first, out_bytes or out_offsets", "NULL out_first")
    refused(calls.fill(bytes=None), "NULL out_first, out_bytes or out_offsets", "NULL out_bytes")
    refused(calls.fill(off=None), "NULL out_first, out_bytes or out_offsets", "NULL out_offsets")
    refused(calls.fill(len=None), "NULL out_len or out_src", "NULL out_len")
    refused(calls.fill(src=None), "NULL out_len or out_src", "NULL out_src")
    refused(calls.fill(out=None), "NULL out_data", "NULL out_data with a capacity")
    refused(calls.fill(first=_p(calls.d_good_first, 2)), "misaligned", "out_first + 2")
    refused(calls.fill(bytes=_p(calls.d_good_bytes, 4)), "misaligned", "out_bytes + 4")
    refused(calls.fill(off=_p(calls.d_off, 4)), "misaligned", "out_offsets + 4")
    refused(calls.fill(len=_p(calls.d_len, 2)), "misaligned", "out_len + 2")
    refused(calls.fill(src=_p(calls.d_src, 1)), "misaligned", "out_src + 1")
    refused(calls.fill(out=_p(calls.d_out, 8)), "misaligned", "out_data + 8")


def test_an_empty_batch_writes_the_totals_and_nothing_else(calls, engine):
    import torch
    empty = FrameBatch.from_packed([], pad_to=1).to_c()
    rc, text, _ = calls.plan(frames=empty, rows=None, ws=None, ws_bytes=0)
    torch.cuda.synchronize()
    first, nbytes = calls.d_first.cpu().numpy(), calls.d_bytes.cpu().numpy()
    assert rc == abi.OK and int(first[:4].view(np.uint32)[0]) == 0 and (first[4:] == FILL).all(), text
    assert int(nbytes[:8].view(np.int64)[0]) == 0 and (nbytes[8:] == FILL).all()
    zero = torch.zeros(1, dtype=torch.int64, device="cuda")
    rc, text, _ = calls.fill(frames=empty, first=_p(calls.d_first), bytes=_p(zero), count=0, len=None, src=None, out=None, cap=0)
    torch.cuda.synchronize()
    off = calls.d_off.cpu().numpy()
    assert rc == abi.OK and int(off[:8].view(np.int64)[0]) == 0 and (off[8:] == FILL).all(), text
    out, src, rows = engine.fragment(FrameBatch.from_packed([], pad_to=1), 1500)
    assert out.count == 0 and src.numel() == 0 and rows.numel() == 0 and out.offsets.cpu().numpy().tolist() == [0]
