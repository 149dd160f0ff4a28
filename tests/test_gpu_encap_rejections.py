"""GPU: what nexg_encap_plan and nexg_encap_frames refuse (include/nexg.h), each
with NEXG_EINVAL and the context's last error set, and nothing launched: the
offsets, lengths, rows, workspace and output keep what they held."""
import ctypes

import numpy as np
import pytest

from nex_amd import abi
from nex_amd.encap import TunnelSet, encap_host, plan_host
from nex_amd.engine import FrameBatch
from tests import encap_frames as ef
from tests.test_encap_host import invalid_sets

pytestmark = pytest.mark.gpu

N = 300
FILL = 0xA5


def _p(t, step=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + step)


class Calls:
    """A valid plan and a valid fill over 300 frames, and variations of them."""

    def __init__(self, engine):
        import torch
        inner = list(ef.small_inner())
        self.engine = engine
        self.frames = [inner[i % len(inner)] for i in range(N)]
        self.batch = FrameBatch.from_packed(self.frames, pad_to=1)
        self.tunnels = ef.spec_sets()[0][0]
        self.index = [i % 17 for i in range(N)]
        self.flows = ef.flows_array(ef.hashes_for(N))
        self.want, self.rows = encap_host(self.frames, self.tunnels, self.index, self.flows)
        self.offs = plan_host([len(w) for w in self.want], 1)
        self.total = int(self.offs[-1])
        u8 = lambda n: torch.full((n,), FILL, dtype=torch.uint8, device="cuda")  # noqa: E731
        self.d_index = torch.tensor(self.index, dtype=torch.uint8, device="cuda")
        self.d_flows = torch.from_numpy(self.flows.view(np.uint8).copy()).cuda()
        self.d_offs, self.d_len, self.d_rows = u8((N + 2) * 8), u8((N + 2) * 4), u8((N + 2) * 8)
        self.ws_bytes = abi.encap_plan_workspace(N)
        self.d_ws = u8(self.ws_bytes + 16)
        self.d_good_offs = torch.from_numpy(self.offs).cuda()
        self.d_out = u8(self.total + 64)

    def _untouched(self, *tensors):
        import torch
        torch.cuda.synchronize()
        return all(bool((t == FILL).all()) for t in tensors)

    def plan(self, **ch):
        a = dict(frames=self.batch.to_c(), set=self.tunnels.to_c(), index=_p(self.d_index), align=1, offs=_p(self.d_offs),
                 len=_p(self.d_len), ws=_p(self.d_ws), ws_bytes=self.ws_bytes)
        a.update(ch)
        for t in (self.d_offs, self.d_len, self.d_ws):
            t.fill_(FILL)
        lib, eng = self.engine.lib, self.engine
        ref = lambda v: None if v is None else ctypes.byref(v)  # noqa: E731
        rc = lib.nexg_encap_plan(eng.ctx, ref(a["frames"]), ref(a["set"]), a["index"], a["align"], a["offs"], a["len"], a["ws"],
                                 a["ws_bytes"], eng._stream(None))
        return rc, lib.nexg_ctx_last_error(eng.ctx).decode(), self._untouched(self.d_offs, self.d_len, self.d_ws)

    def fill(self, **ch):
        a = dict(frames=self.batch.to_c(), set=self.tunnels.to_c(), index=_p(self.d_index), flows=_p(self.d_flows),
                 offs=_p(self.d_good_offs), out=_p(self.d_out), cap=self.total, rows=_p(self.d_rows))
        a.update(ch)
        for t in (self.d_out, self.d_rows):
            t.fill_(FILL)
        lib, eng = self.engine.lib, self.engine
        ref = lambda v: None if v is None else ctypes.byref(v)  # noqa: E731
        rc = lib.nexg_encap_frames(eng.ctx, ref(a["frames"]), ref(a["set"]), a["index"], a["flows"], a["offs"], a["out"],
                                   a["cap"], a["rows"], eng._stream(None))
        return rc, lib.nexg_ctx_last_error(eng.ctx).decode(), self._untouched(self.d_out, self.d_rows)

    def table(self, **kw):
        fr = self.batch.to_c()
        for k, v in kw.items():
            setattr(fr, k, v)
        return fr


@pytest.fixture(scope="module")
def calls(engine, oracle):
    return Calls(engine)


def refused(result, text, what):
    rc, got, untouched = result
    assert rc == abi.EINVAL and text in got and untouched, (what, rc, got, untouched)


def test_the_valid_calls_are_accepted(calls):
    rc, text, untouched = calls.plan()
    assert rc == abi.OK and not untouched, text
    offs = calls.d_offs.cpu().numpy()
    assert (offs[: (N + 1) * 8].view(np.int64) == calls.offs).all() and (offs[(N + 1) * 8:] == FILL).all()
    lens = calls.d_len.cpu().numpy()
    assert (lens[: N * 4].view(np.uint32) == [len(w) for w in calls.want]).all() and (lens[N * 4:] == FILL).all()
    assert (calls.d_ws.cpu().numpy()[calls.ws_bytes:] == FILL).all()
    rc, text, untouched = calls.fill()
    assert rc == abi.OK and not untouched, text
    out = calls.d_out.cpu().numpy()
    assert out[: calls.total].tobytes() == b"".join(calls.want) and (out[calls.total:] == FILL).all()
    rows = calls.d_rows.cpu().numpy()
    assert (rows[: N * 8].view(abi.ENCAPPED_DTYPE) == calls.rows).all() and (rows[N * 8:] == FILL).all()
    rc, text, _ = calls.plan(len=None)  # optional
    assert rc == abi.OK, text
    rc, text, _ = calls.fill(rows=None)
    assert rc == abi.OK and calls.d_out.cpu().numpy()[: calls.total].tobytes() == b"".join(calls.want), text


def test_invalid_sets_are_refused_by_both(calls):
    for name, c in invalid_sets().items():
        refused(calls.plan(set=c), "encap_plan: ", name)
        refused(calls.fill(set=c), "encap_frames: ", name)
    refused(calls.plan(set=None), "NULL tunnel set", "NULL set")
    refused(calls.fill(set=None), "NULL tunnel set", "NULL set")


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


def test_plan_arguments(calls):
    for align in (0, 2, 3, 5, 32):
        refused(calls.plan(align=align), "align must be 1, 4, 8 or 16", f"align {align}")
    refused(calls.plan(offs=None), "NULL out_offsets", "NULL out_offsets")
    refused(calls.plan(ws=None), "NULL workspace", "NULL workspace")
    refused(calls.plan(ws_bytes=calls.ws_bytes - 1), "workspace smaller than nexg_encap_plan_workspace", "small workspace")
    refused(calls.plan(offs=_p(calls.d_offs, 4)), "misaligned output or workspace", "out_offsets + 4")
    refused(calls.plan(ws=_p(calls.d_ws, 4)), "misaligned output or workspace", "workspace + 4")
    refused(calls.plan(len=_p(calls.d_len, 2)), "misaligned output or workspace", "out_len + 2")


def test_fill_arguments(calls):
    refused(calls.fill(flows=None), "FLOW_PORT and flows is NULL", "FLOW_PORT without flows")
    refused(calls.fill(offs=None), "NULL out_offsets", "NULL out_offsets")
    refused(calls.fill(out=None), "NULL out_data", "NULL out_data with a capacity")
    refused(calls.fill(offs=_p(calls.d_good_offs, 4)), "misaligned", "out_offsets + 4")
    refused(calls.fill(flows=_p(calls.d_flows, 4)), "misaligned", "flows + 4")
    refused(calls.fill(rows=_p(calls.d_rows, 4)), "misaligned", "rows + 4")
    refused(calls.fill(out=_p(calls.d_out, 8)), "misaligned", "out_data + 8")
    # flows may be NULL when no spec asks for them
    plain = TunnelSet([ef.specs()[2], ef.specs()[8]]).to_c()
    rc, text, _ = calls.fill(set=plain, flows=None)
    assert rc == abi.OK, text


def test_an_empty_batch_launches_nothing_but_the_total(calls):
    import torch
    empty = FrameBatch.from_packed([], pad_to=1).to_c()
    rc, text, _ = calls.plan(frames=empty, index=None, ws=None, ws_bytes=0, len=None)
    torch.cuda.synchronize()
    offs = calls.d_offs.cpu().numpy()
    assert rc == abi.OK and int(offs[:8].view(np.int64)[0]) == 0 and (offs[8:] == FILL).all(), text
    rc, text, untouched = calls.fill(frames=empty, index=None, offs=None, out=None, cap=0, rows=None)
    assert rc == abi.OK and untouched, text
