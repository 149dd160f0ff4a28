"""The C++ host API's fragmentation (include/nexg.hpp nexg::FragOption,
Engine::fragment_plan, fragment, fragment_bufs;
tests/native/cpp_fragment_test.cpp). CPU: the wrappers compile with -Wall
-Werror and link against libnexg.so, the builder refuses what
nexg_frag_option_check refuses, and the workspace's regions fit the header's
size. GPU: the corpus's small frames under two options give the output
frames, the table and the rows of fragment_host."""
import subprocess

import pytest

from nex_amd import abi
from nex_amd.fragment import fragment_host, plan_host
from tests import fragment_frames as ff

from tests.helpers import build_native_test  # __graft_entry__.build() makes it too


def test_cpp_fragment_compiles_links_and_refuses():
    exe = build_native_test("cpp_fragment_test")
    r = subprocess.run([exe, "--link"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["link", "ok", "3", "3", "7", "8"]


@pytest.mark.gpu
def test_cpp_fragment_gpu(engine, tmp_path):
    exe = build_native_test("cpp_fragment_test")
    frames = [f for f in ff.frames() if f is not None and len(f) < 4096]
    p = tmp_path / "frames.txt"
    p.write_text("".join((f.hex() or "-") + "\n" for f in frames))
    r = subprocess.run([exe, "--gpu", str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    it = iter(l.split() for l in r.stdout.splitlines())
    for mtu, ignore_df, align in ((576, False, 1), (1500, True, 16)):
        pieces, src, rows = fragment_host(frames, mtu, ignore_df)
        # DF frames and IPv6 at 576; under IGNORE_DF only IPv6 is left to report
        assert int((rows["kind"] == abi.FRAG_SPLIT).sum()) >= 20 and int((rows["kind"] == abi.FRAG_TOO_BIG).sum()) >= (1 if ignore_df else 3)
        offs = plan_host([len(x) for x in pieces], align)
        assert next(it) == ["W", str(mtu), str(align), str(len(frames)), str(len(pieces)), str(int(offs[-1]))]
        for i, row in enumerate(rows):
            assert next(it) == ["R"] + [str(int(row[n])) for n in ("status", "kind", "hdr_len", "pieces", "piece_data", "first")], (mtu, i)
        for f, x in enumerate(pieces):
            assert next(it) == ["F", str(int(offs[f])), str(int(src[f])), x.hex() or "-"], (mtu, f)
    assert next(it, None) is None
