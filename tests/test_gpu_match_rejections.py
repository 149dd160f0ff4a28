"""GPU: what nexg_match_batch and nexg_match_select refuse (include/nexg.h),
each with NEXG_EINVAL and the context's last error set, and nothing launched:
every output and the workspace keep the pattern they were filled with."""
import ctypes

import numpy as np
import pytest

from nex_amd import abi
from nex_amd.engine import FrameBatch
from nex_amd.match import Pattern, PatternSet
from tests import match_frames as mf

pytestmark = pytest.mark.gpu

N = 300
FILL = 0xA5


def _p(t, step=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + step)


class Calls:
    """A valid call of each entry over 300 frames, and variations of it."""

    def __init__(self, engine, oracle):
        import torch
        c = mf.case("nocase")
        which = np.arange(N) % len(c.frames)
        self.engine = engine
        self.batch = FrameBatch.from_packed([c.frames[i] for i in which], pad_to=1)
        recs, rows = mf.expected(oracle, c)
        self.pset = c.pset
        self.want_rows = rows[which]
        self.recs = torch.from_numpy(recs[which].view(np.uint8).copy()).cuda()
        self.rows = torch.from_numpy(rows[which].view(np.uint8).copy()).cuda()
        self.wsb = abi.match_select_workspace(N)
        self.t = dict(out=torch.empty((N + 2) * 8, dtype=torch.uint8, device="cuda"),
                      idx=torch.empty(N + 4, dtype=torch.int32, device="cuda"),
                      off=torch.empty(N + 4, dtype=torch.int64, device="cuda"),
                      ln=torch.empty(N + 4, dtype=torch.int32, device="cuda"),
                      cnt=torch.empty(2, dtype=torch.int64, device="cuda"),
                      ws=torch.empty(self.wsb + 16, dtype=torch.uint8, device="cuda"))

    def _run(self, call):
        import torch
        for t in self.t.values():
            t.view(torch.uint8).fill_(FILL)
        lib, eng = self.engine.lib, self.engine
        rc = call(lib, eng)
        torch.cuda.synchronize()
        untouched = all(bool((t.view(torch.uint8) == FILL).all()) for t in self.t.values())
        return rc, lib.nexg_ctx_last_error(eng.ctx).decode(), untouched

    def match(self, **ch):
        a = dict(frames=self.batch.to_c(), recs=_p(self.recs), set=self.pset.to_c(), out=_p(self.t["out"]))
        a.update(ch)
        return self._run(lambda lib, eng: lib.nexg_match_batch(
            eng.ctx, None if a["frames"] is None else ctypes.byref(a["frames"]), a["recs"],
            None if a["set"] is None else ctypes.byref(a["set"]), a["out"], eng._stream(None)))

    def select(self, **ch):
        a = dict(frames=self.batch.to_c(), rows=_p(self.rows), masks=(1, 0, 0), idx=_p(self.t["idx"]), off=_p(self.t["off"]),
                 ln=_p(self.t["ln"]), cnt=_p(self.t["cnt"]), ws=_p(self.t["ws"]), wsb=self.wsb)
        a.update(ch)
        return self._run(lambda lib, eng: lib.nexg_match_select(
            eng.ctx, None if a["frames"] is None else ctypes.byref(a["frames"]), a["rows"], *a["masks"], a["idx"], a["off"],
            a["ln"], a["cnt"], a["ws"], a["wsb"], eng._stream(None)))


@pytest.fixture(scope="module")
def calls(engine, oracle):
    return Calls(engine, oracle)


def refused(result, text, what):
    rc, got, untouched = result
    assert rc == abi.EINVAL and text in got and untouched, (what, rc, got, untouched)


def bad_tables(batch):
    """Frame tables frames_valid refuses, and a count above 2^32 - 1."""
    def table(**kw):
        fr = batch.to_c()
        for k, v in kw.items():
            setattr(fr, k, v)
        return fr
    return {"NULL data": (table(data=None), "invalid frame batch"),
            "misaligned data": (table(data=batch.data.data_ptr() + 1), "invalid frame batch"),
            "no offsets, no stride": (table(offsets=None, stride=0), "invalid frame batch"),
            "count 2^32": (table(count=1 << 32), "more than 2^32 - 1 frames")}


def test_the_valid_calls_are_accepted(calls):
    import torch
    rc, text, untouched = calls.match()
    assert rc == abi.OK and not untouched, text
    got = calls.t["out"].cpu().numpy()
    assert (got[: N * 8].view(abi.MATCH_DTYPE) == calls.want_rows).all() and (got[N * 8:] == FILL).all()
    rc, text, untouched = calls.select()
    assert rc == abi.OK and not untouched, text
    assert int(calls.t["cnt"][0]) == int((calls.want_rows["mask"] & 1 != 0).sum()) > 0
    assert int(calls.t["cnt"].view(torch.uint8)[8]) == FILL


def test_match_refuses_invalid_sets(calls):
    for name, s in mf.invalid_sets().items():
        refused(calls.match(set=s.to_c(validate=False)), "match: pattern", name)
    refused(calls.match(set=None), "NULL pattern set", "NULL set")
    refused(calls.match(set=PatternSet([Pattern(b"ab", offset=(5, 4))]).to_c(validate=False)), "off_lo > off_hi", "text")


def test_match_refuses_tables_and_pointers(calls):
    for name, (fr, text) in bad_tables(calls.batch).items():
        refused(calls.match(frames=fr), text, name)
    refused(calls.match(frames=None), "", "NULL frames")
    refused(calls.match(recs=None), "NULL records without NEXG_MATCH_FRAME", "NULL records")
    refused(calls.match(recs=_p(calls.recs, 8)), "misaligned", "records + 8")
    refused(calls.match(out=None), "NULL output", "NULL out")
    refused(calls.match(out=_p(calls.t["out"], 4)), "misaligned", "out + 4")
    whole = PatternSet(calls.pset.patterns, frame=True).to_c()
    refused(calls.match(set=whole, recs=None, out=None), "NULL output", "NULL out, whole frame")
    rc, text, untouched = calls.match(set=whole, recs=None)  # the whole frame needs no records
    assert rc == abi.OK and not untouched, text
    rc, text, untouched = calls.match(set=whole, recs=_p(calls.recs, 1))  # ... and does not look at the pointer
    assert rc == abi.OK and not untouched, text


def test_match_select_refusals(calls):
    for name, (fr, text) in bad_tables(calls.batch).items():
        refused(calls.select(frames=fr), text, name)
    refused(calls.select(frames=None), "", "NULL frames")
    for key in ("rows", "idx", "off", "ln", "cnt", "ws"):
        refused(calls.select(**{key: None}), "NULL", key)
    for key, t, step in (("rows", calls.rows, 4), ("off", calls.t["off"], 4), ("cnt", calls.t["cnt"], 4),
                         ("idx", calls.t["idx"], 2), ("ln", calls.t["ln"], 1), ("ws", calls.t["ws"], 2)):
        refused(calls.select(**{key: _p(t, step)}), "misaligned", key)
    refused(calls.select(wsb=calls.wsb - 1), "workspace smaller than nexg_match_select_workspace", "short workspace")
    refused(calls.select(wsb=0), "workspace smaller", "no workspace bytes")


def test_empty_batches(calls, engine):
    """count == 0: the match launches nothing and needs no pointer; the
    selection writes *out_count = 0 and nothing else."""
    import torch
    empty = FrameBatch.from_packed([], pad_to=1).to_c()
    rc, text, untouched = calls.match(frames=empty, recs=None, out=None)
    assert rc == abi.OK and untouched, text
    rc, text, _ = calls.select(frames=empty, rows=None, idx=None, off=None, ln=None, ws=None, wsb=0)
    assert rc == abi.OK, text
    assert int(calls.t["cnt"][0]) == 0
    for k in ("out", "idx", "off", "ln", "ws"):
        assert bool((calls.t[k].view(torch.uint8) == FILL).all()), k
    with pytest.raises(ValueError):
        engine.match_select(calls.batch, calls.rows, any=1 << 32)
