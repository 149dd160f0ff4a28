"""The C++ host API's fixed-string match (include/nexg.hpp nexg::PatternSet,
Engine::match, match_select, match_bufs; tests/native/cpp_match_test.cpp).
CPU: the wrappers compile with -Wall -Werror and link against libnexg.so, and
the builder refuses what nexg_patterns_check refuses. GPU: two sets over a
small corpus give the rows match_rows_host gives on the oracle's records, and
the selection match_select_host gives."""
import subprocess

import numpy as np
import pytest

from nex_amd import abi
from nex_amd import match as M
from nex_amd.match import Pattern, PatternSet
from tests import match_frames as mf

from tests.helpers import build_native_test  # __graft_entry__.build() makes it too


def test_cpp_match_compiles_and_links():
    exe = build_native_test("cpp_match_test")
    r = subprocess.run([exe, "--link"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["link", "ok", "3", "3", "1", "2", "9", str(abi.match_select_workspace(65793))]


def small_corpus():
    frames = []
    for name in ("nocase", "windows", "header trap payload", "empty regions"):
        frames += mf.case(name).frames
    frames += [mf.udp(b"GET / HTTP/1.1\r\nhost: x"), mf.udp(b"GET /mark"), mf.udp(b"." * 21 + b"mark"), mf.tcp(b"GET xyz"), b""]
    return frames


@pytest.mark.gpu
def test_cpp_match_gpu(oracle, tmp_path):
    exe = build_native_test("cpp_match_test")
    frames = small_corpus()
    recs = oracle.parse_frames(frames, mf.PARSE_FLAGS)
    p = tmp_path / "frames.txt"
    p.write_text("".join((f.hex() or "-") + "\n" for f in frames))
    r = subprocess.run([exe, "--gpu", str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    sets = [(PatternSet([Pattern(b"hOsT:", nocase=True), Pattern.prefix(b"GET "), Pattern(b"mark", offset=(20, 22))]),
             dict(any=0x5, none=0x2)),
            (PatternSet([Pattern(bytes(range(1, 7)), offset=(0, 0)), Pattern(b"xyz")], frame=True), dict(all=0x3))]
    offs = np.cumsum([0] + [(len(f) + 3) // 4 * 4 for f in frames])[:-1]  # HostBatch: each start 4-B aligned
    it = iter(l.split() for l in r.stdout.splitlines())
    for si, (pset, kw) in enumerate(sets):
        rows = M.match_rows_host(frames, recs, [len(f) for f in frames], pset)
        pick = M.match_select_host(rows, **kw)
        assert 0 < len(pick) < len(frames), si
        assert next(it) == ["M", str(si), str(len(frames)), str(len(pick))]
        for i, row in enumerate(rows):
            assert next(it) == ["R", f"{int(row['mask']):08x}", str(int(row["first_off"])), str(int(row["first_pat"]))], (si, i)
        for i in pick:
            assert next(it) == ["S", str(i), str(int(offs[i])), str(len(frames[i]))], (si, i)
    assert next(it, None) is None
