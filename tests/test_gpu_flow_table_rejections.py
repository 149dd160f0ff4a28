"""GPU: what nexg_flow_table_merge refuses (include/nexg.h), each with
NEXG_EINVAL and its text, and nothing written: table_out, out_slot,
*out_count and the workspace keep the pattern they were filled with."""
import ctypes

import numpy as np
import pytest

from nex_amd import abi
from nex_amd.engine import FrameBatch
from nex_amd.flow import FlowOption
from tests.test_gpu_flow_table import _p, dev, hash_sets, made_up_groups, made_up_table

pytestmark = pytest.mark.gpu

N_IN, N_G = 300, 200


class Call:
    """A valid call on made-up rows and an empty frame table, and variations of it."""

    def __init__(self, engine):
        import torch
        rng = np.random.default_rng(3)
        a, b = hash_sets(rng, N_IN, N_G)
        self.engine = engine
        self.batch = FrameBatch.from_packed([], pad_to=1)
        self.wsb = abi.flow_table_workspace(N_IN, N_G)
        self.t = dict(groups=dev(made_up_groups(np.sort(b), rng)), table_in=dev(made_up_table(np.sort(a), rng)),
                      table_out=torch.empty((N_IN + N_G + 1) * 64, dtype=torch.uint8, device="cuda"),
                      out_slot=torch.empty(N_G + 4, dtype=torch.int32, device="cuda"),
                      out_count=torch.empty(4, dtype=torch.int64, device="cuda"),
                      workspace=torch.empty(self.wsb // 8 + 2, dtype=torch.int64, device="cuda"))
        self.outputs = ("table_out", "out_slot", "out_count", "workspace")
        self.good = dict(frames=self.batch.to_c(), records=None, option=None, groups=_p(self.t["groups"]), n_groups=N_G,
                         table_in=_p(self.t["table_in"]), n_in=N_IN, epoch=4, min_epoch=2,
                         table_out=_p(self.t["table_out"]), table_cap=N_IN + N_G, out_slot=_p(self.t["out_slot"]),
                         out_count=_p(self.t["out_count"]), workspace=_p(self.t["workspace"]), workspace_bytes=self.wsb)

    def moved(self, name, step):
        return ctypes.c_void_p(self.t[name].data_ptr() + step)

    def run(self, **changes):
        """(status, error text, whether every output still holds its fill)."""
        import torch
        for n in self.outputs:
            self.t[n].view(torch.uint8).fill_(0xA5)
        a = dict(self.good, **changes)
        lib, eng = self.engine.lib, self.engine
        rc = lib.nexg_flow_table_merge(eng.ctx, ctypes.byref(a["frames"]), a["records"],
                                       None if a["option"] is None else ctypes.byref(a["option"]), a["groups"],
                                       a["n_groups"], a["table_in"], a["n_in"], a["epoch"], a["min_epoch"], a["table_out"],
                                       a["table_cap"], a["out_slot"], a["out_count"], a["workspace"], a["workspace_bytes"],
                                       eng._stream(None))
        torch.cuda.synchronize()
        untouched = all(bool((self.t[n].view(torch.uint8) == 0xA5).all()) for n in self.outputs)
        return rc, lib.nexg_ctx_last_error(eng.ctx).decode(), untouched


@pytest.fixture(scope="module")
def call(engine):
    return Call(engine)


def test_the_valid_call_is_accepted(call):
    rc, text, untouched = call.run()
    assert rc == abi.OK and not untouched, text


def refused(call, text, **changes):
    rc, got, untouched = call.run(**changes)
    assert rc == abi.EINVAL and text in got and untouched, (changes.keys(), rc, got, untouched)


def test_option(call):
    refused(call, "unknown flag bits", option=FlowOption(flags=0x8).to_c(validate=False))
    refused(call, "reserved must be 0", option=FlowOption(reserved=1).to_c(validate=False))


def test_null_pointers(call):
    for name in ("groups", "table_in", "table_out", "out_count", "workspace"):
        refused(call, "NULL", **{name: None})
    # records are needed once the frame table has frames
    frames = call.batch.to_c()
    frames.count, frames.stride, frames.offsets, frames.lengths = 1, 64, None, None
    frames.data, frames.data_bytes = call.t["workspace"].data_ptr(), 64
    refused(call, "NULL", frames=frames)


def test_misaligned_pointers(call):
    for name, step in (("groups", 8), ("table_in", 8), ("table_out", 8), ("out_count", 4), ("workspace", 4),
                       ("out_slot", 2)):
        refused(call, "misaligned", **{name: call.moved(name, step)})
    refused(call, "misaligned", records=ctypes.c_void_p(call.t["workspace"].data_ptr() + 8))


def test_table_out_overlapping_table_in(call):
    n = N_IN * 64
    for out, cap in ((call.good["table_in"], N_IN + N_G), (call.moved("table_in", n - 64), 1),
                     (call.moved("table_in", 64), 1 << 60)):
        refused(call, "overlaps", table_out=out, table_cap=cap)
    # ... from below: the last row of table_out would be table_in's first
    refused(call, "overlaps", table_in=call.moved("table_out", 64 * N_G), table_cap=N_G + 1)
    # side by side is fine
    rc, text, _ = call.run(table_in=call.moved("table_out", 64 * (N_G + 1)), n_in=N_IN - 1, table_cap=N_G + 1)
    assert rc == abi.OK, text


def test_counts_above_2_31_minus_1(call):
    huge = abi.flow_table_workspace(1 << 31, 1 << 31)
    refused(call, "2^31 - 1", n_in=1 << 31, workspace_bytes=huge)
    refused(call, "2^31 - 1", n_groups=1 << 31, workspace_bytes=huge)
    refused(call, "2^31 - 1", n_groups=(1 << 64) - 1)


def test_invalid_frame_table(call):
    frames = call.batch.to_c()
    frames.count, frames.data = 5, None
    refused(call, "invalid frame batch", frames=frames)


def test_short_workspace(call):
    refused(call, "workspace smaller than nexg_flow_table_workspace", workspace_bytes=call.wsb - 1)
    refused(call, "workspace smaller than nexg_flow_table_workspace", workspace_bytes=0)


def test_no_context(call):
    import torch
    a = call.good
    for n in call.outputs:
        call.t[n].view(torch.uint8).fill_(0xA5)
    rc = call.engine.lib.nexg_flow_table_merge(None, ctypes.byref(a["frames"]), None, None, a["groups"], N_G, a["table_in"],
                                               N_IN, 4, 2, a["table_out"], N_IN + N_G, a["out_slot"], a["out_count"],
                                               a["workspace"], call.wsb, call.engine._stream(None))
    torch.cuda.synchronize()
    assert rc == abi.EINVAL and all(bool((call.t[n].view(torch.uint8) == 0xA5).all()) for n in call.outputs)


def test_empty_inputs_write_the_count_and_nothing_else(call):
    import torch
    rc, text, _ = call.run(n_in=0, n_groups=0, table_in=None, groups=None, workspace=None, workspace_bytes=0,
                           table_out=None, table_cap=0, out_slot=None)
    assert rc == abi.OK, text
    assert call.t["out_count"].cpu().tolist()[0] == 0
    assert bool((call.t["out_count"][1:].view(torch.uint8) == 0xA5).all())
    for n in ("table_out", "out_slot", "workspace"):
        assert bool((call.t[n].view(torch.uint8) == 0xA5).all()), n
