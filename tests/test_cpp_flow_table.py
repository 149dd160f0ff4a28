"""GPU: the flow table through the C++ host API (include/nexg.hpp
nexg::FlowEntry, Engine::flow_table_merge / flow_table_bufs): the corpus with
the collision pair cut into three batches and merged one after the other by
tests/native/cpp_flow_table_test, against nex_amd.flow.merge_host on the
oracle's records, as tests/test_gpu_flow_groups.py does for the groups."""
import subprocess

import numpy as np
import pytest

from nex_amd import abi
from nex_amd.flow import FlowOption, flows_host, groups_host, merge_host
from tests import flow_frames as ff
from tests import flow_group_frames as fg
from tests.helpers import build_native_test

pytestmark = pytest.mark.gpu

SIZES = (40, 65)  # the third batch takes the rest


def test_cpp_flow_table_gpu(oracle, tmp_path):
    exe = build_native_test("cpp_flow_table_test")
    frames = [x.frame for x in ff.small_corpus()] + fg.collision_frames()
    assert len(frames) > sum(SIZES) + 5
    recs = oracle.parse_frames(frames, ff.PARSE_FLAGS)
    lengths = np.array([len(f) for f in frames])
    p = tmp_path / "frames.txt"
    p.write_text("".join((f.hex() or "-") + "\n" for f in frames))
    r = subprocess.run([exe, "--gpu", str(p)] + [str(s) for s in SIZES], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    it = iter(l.split() for l in r.stdout.splitlines())
    cuts = [0, SIZES[0], SIZES[0] + SIZES[1], len(frames)]
    for oi, opt in enumerate((FlowOption(), FlowOption(symmetric=True))):
        flows = flows_host(frames, recs, lengths, opt)
        table = np.zeros(0, abi.FLOW_ENTRY_DTYPE)
        for epoch in range(3):
            w = slice(cuts[epoch], cuts[epoch + 1])
            groups, group_of, _ = groups_host(frames[w], recs[w], lengths[w], flows[w], opt)
            table, slot = merge_host(table, groups, frames[w], recs[w], lengths[w], opt, epoch, 0)
            assert next(it) == ["T", str(oi), str(epoch), str(len(table))]
            for e in table:
                assert next(it) == ["E", f"{int(e['hash']):08x}", str(int(e["kind"])), str(int(e["proto"])),
                                    str(int(e["flags8"])), "0", bytes(e["key"]).hex(), str(int(e["last_epoch"])),
                                    str(int(e["packets"])), str(int(e["bytes"]))], (oi, epoch, e)
            assert next(it) == ["S"] + [str(int(s)) for s in slot], (oi, epoch)
            assert next(it) == ["M"] + [str(int(g)) for g in group_of], (oi, epoch)
        assert int(table["packets"].sum()) == len(frames) and int(table["flags8"].sum()) >= 1
    assert next(it, None) is None
