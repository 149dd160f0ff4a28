"""The C++ host API's frame selection and gather (include/nexg.hpp
nexg::Filter, Engine::select, gather_plan, gather, gather_rows, select_bufs;
tests/native/cpp_select_test.cpp). CPU: the wrappers compile with -Wall
-Werror and link against libnexg.so, and the builder refuses what
nexg_filter_check refuses. GPU: three filters over the selection corpus give
the indices, rules, records and gathered bytes that match_host / gather_host
give on the oracle's records."""
import subprocess

import numpy as np
import pytest

from nex_amd import abi
from nex_amd import select as S
from nex_amd.select import Filter, Rule

from tests.helpers import build_native_test  # __graft_entry__.build() makes it too


def test_cpp_select_compiles_and_links():
    exe = build_native_test("cpp_select_test")
    r = subprocess.run([exe, "--link"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["link", "ok", "5", "5", "3", "3", str(abi.select_workspace(65793)),
                                str(abi.gather_plan_workspace(65793))]


@pytest.mark.gpu
def test_cpp_select_gpu(oracle, tmp_path):
    from tests import select_frames as sf
    exe = build_native_test("cpp_select_test")
    frames = [x.frame for x in sf.small_corpus()]
    recs = oracle.parse_frames(frames, sf.PARSE_FLAGS)
    p = tmp_path / "frames.txt"
    p.write_text("".join((f.hex() or "-") + "\n" for f in frames))
    r = subprocess.run([exe, "--gpu", str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l.split() for l in r.stdout.splitlines()]
    filters = [sf.FILTERS["issue examples"], Filter([Rule.udp() & Rule.length(0, 100)], invert=True),
               Filter([Rule.status(abi.ERR_TRUNCATED), Rule.proto(58)])]
    # the layout HostBatch builds: frames back to back, each start 4-B aligned
    offs = np.cumsum([0] + [(len(f) + 3) // 4 * 4 for f in frames])[:-1]
    data = np.zeros(int(offs[-1]) + len(frames[-1]) + 4, np.uint8)
    for o, f in zip(offs, frames):
        data[o:o + len(f)] = np.frombuffer(f, np.uint8)
    it = iter(lines)
    for fi, flt in enumerate(filters):
        idx, rule = S.select_host(frames, recs, [len(f) for f in frames], flt)
        assert 0 < len(idx) < len(frames), fi
        for align in (1, 4, 16):
            go, gl, gd = S.gather_host(data, offs[idx], [len(frames[i]) for i in idx], align)
            head = next(it)
            assert head == ["F", str(fi), str(align), str(len(idx)), str(len(gd))], (fi, align, head)
            for k, i in enumerate(idx):
                s = next(it)
                want = gd[int(go[k]): int(go[k + 1])].tobytes().hex()
                assert s[:6] == ["S", str(i), str(rule[k]), str(int(go[k])), str(int(gl[k])),
                                 f"{int(recs[i]['flags']):08x}"], (fi, align, k, s[:6])
                assert (s[6] if len(s) > 6 else "") == want, (fi, align, k)
    assert next(it, None) is None
