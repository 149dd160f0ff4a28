"""The C++ host API's header rewrite (include/nexg.hpp nexg::Action,
nexg::ActionSet, Engine::rewrite, rewrite_bufs; tests/native/cpp_rewrite_test.cpp).
CPU: the wrappers compile with -Wall -Werror and link against libnexg.so, and
the builders refuse what nexg_actions_check refuses. GPU: three actions, the
index cycling through them and past the set, give the bytes and rows
rewrite_host gives on the corpus, in both checksum modes."""
import subprocess

import pytest

from nex_amd import abi
from nex_amd.rewrite import Action, ActionSet, rewrite_host
from tests import rewrite_frames as rf

from tests.helpers import build_native_test  # __graft_entry__.build() makes it too


def test_cpp_rewrite_compiles_links_and_refuses():
    exe = build_native_test("cpp_rewrite_test")
    r = subprocess.run([exe, "--link"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["link", "ok", "2", "3", "13"]


def actions(incremental):
    return ActionSet([Action.nat4(src=rf.S4[:4], dst=rf.D4[:4]) & Action.ports(40000, 443) & Action.dec_ttl(1),
                      Action.nat6(src=rf.S6, dst=rf.D6) & Action.ports(src=9) & Action.set_tos(0x28, 0xFC) &
                      Action.mac(dst=rf.M1, src=rf.M2),
                      Action.set_ttl(7)], incremental=incremental)


@pytest.mark.gpu
def test_cpp_rewrite_gpu(oracle, tmp_path):
    exe = build_native_test("cpp_rewrite_test")
    c = rf.corpus()
    frames = [h[i] for h in (c.fixed, c.garbage) for i in rf.small(h)]
    index = [abi.ACTION_NONE if i % 5 == 4 else i % 5 for i in range(len(frames))]
    p = tmp_path / "frames.txt"
    p.write_text("".join((f.hex() or "-") + "\n" for f in frames))
    r = subprocess.run([exe, "--gpu", str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    it = iter(l.split() for l in r.stdout.splitlines())
    for mode in (0, 1):
        want, rows = rewrite_host(frames, actions(bool(mode)), index)
        assert int((rows["fixed"] == rf.BOTH).sum()) >= 50 and int((rows["action"] == abi.ACTION_NONE).sum()) >= 50
        assert next(it) == ["W", str(mode), str(len(frames))]
        for i, (w, row) in enumerate(zip(want, rows)):
            assert next(it) == ["F", w.hex() or "-"] + [str(v) for v in rf.row_tuple(row)], (mode, i)
    assert next(it, None) is None
