"""GPU: what nexg_rewrite_batch refuses (include/nexg.h), each with NEXG_EINVAL
and the context's last error set, and nothing launched: the data buffer and
the rows keep what they held."""
import ctypes

import numpy as np
import pytest

from nex_amd import abi
from nex_amd.engine import FrameBatch
from tests import rewrite_frames as rf
from tests.test_rewrite_host import invalid_sets

pytestmark = pytest.mark.gpu

N = 300
FILL = 0xA5


def _p(t, step=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + step)


class Calls:
    """A valid call over 300 frames, and variations of it."""

    def __init__(self, engine):
        import torch
        c = rf.corpus()
        pool = [c.garbage[i] for i in rf.small(c.garbage) if len(c.garbage[i]) >= 42]
        self.engine = engine
        self.frames = [pool[i % len(pool)] for i in range(N)]
        self.batch = FrameBatch.from_packed(self.frames, pad_to=1)
        self.before = self.batch.data.clone()
        self.actions = rf.to_set([rf.NAT44])
        self.index = torch.zeros(N, dtype=torch.uint8, device="cuda")
        self.out = torch.empty((N + 2) * 8, dtype=torch.uint8, device="cuda")
        self.opt = abi.ParseOptionC(0, 0)

    def rewrite(self, **ch):
        import torch
        a = dict(frames=self.batch.to_c(), opt=self.opt, actions=self.actions.to_c(), index=_p(self.index), out=_p(self.out))
        a.update(ch)
        self.batch.data.copy_(self.before)
        self.out.fill_(FILL)
        lib, eng = self.engine.lib, self.engine
        ref = lambda v: None if v is None else ctypes.byref(v)  # noqa: E731
        rc = lib.nexg_rewrite_batch(eng.ctx, ref(a["frames"]), ref(a["opt"]), ref(a["actions"]), a["index"], a["out"],
                                    eng._stream(None))
        torch.cuda.synchronize()
        untouched = bool((self.batch.data == self.before).all()) and bool((self.out == FILL).all())
        return rc, lib.nexg_ctx_last_error(eng.ctx).decode(), untouched


@pytest.fixture(scope="module")
def calls(engine, oracle):
    return Calls(engine)


def refused(result, text, what):
    rc, got, untouched = result
    assert rc == abi.EINVAL and text in got and untouched, (what, rc, got, untouched)


def test_the_valid_call_is_accepted(calls):
    from nex_amd.rewrite import rewrite_host
    rc, text, untouched = calls.rewrite()
    assert rc == abi.OK and not untouched, text
    want, rows = rewrite_host(calls.frames, calls.actions)
    assert calls.batch.data.cpu().numpy()[: sum(map(len, want))].tobytes() == b"".join(want)
    got = calls.out.cpu().numpy()
    assert (got[: N * 8].view(abi.REWRITTEN_DTYPE) == rows).all() and (got[N * 8:] == FILL).all()
    rc, text, untouched = calls.rewrite(index=None, out=None)  # both are optional
    assert rc == abi.OK and calls.batch.data.cpu().numpy()[: sum(map(len, want))].tobytes() == b"".join(want), text


def test_invalid_sets_leave_the_data_untouched(calls):
    for name, s in invalid_sets().items():
        c = s.to_c(validate=False)
        if name == "n_actions 17":
            c.n_actions = 17
        refused(calls.rewrite(actions=c), "rewrite: ", name)
    refused(calls.rewrite(actions=None), "NULL action set", "NULL actions")


def test_tables_and_pointers(calls):
    def table(**kw):
        fr = calls.batch.to_c()
        for k, v in kw.items():
            setattr(fr, k, v)
        return fr
    for name, fr in {"NULL data": table(data=None), "misaligned data": table(data=calls.batch.data.data_ptr() + 1),
                     "no offsets, no stride": table(offsets=None, stride=0)}.items():
        refused(calls.rewrite(frames=fr), "invalid frame batch", name)
    refused(calls.rewrite(frames=None), "invalid frame batch", "NULL frames")
    refused(calls.rewrite(opt=None), "NULL option", "NULL option")
    refused(calls.rewrite(out=_p(calls.out, 4)), "misaligned output", "out + 4")


def test_an_empty_batch_launches_nothing(calls):
    empty = FrameBatch.from_packed([], pad_to=1).to_c()
    rc, text, untouched = calls.rewrite(frames=empty, index=None)
    assert rc == abi.OK and untouched, text
