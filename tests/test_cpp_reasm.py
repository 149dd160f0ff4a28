"""The C++ host API's reassembly (include/nexg.hpp Engine::reassemble_plan,
reassemble, reassemble_held, reassemble_bufs;
tests/native/cpp_reasm_test.cpp). CPU: the wrappers compile with -Wall -Werror
and link against libnexg.so, and the workspace's regions fit the header's
size. GPU: a corpus table at align 1 and 16 gives the output frames, the
table, the rows and the held frames of reassemble_host."""
import subprocess

import numpy as np
import pytest

from nex_amd import abi
from nex_amd.reassemble import pack_host, reassemble_host
from tests import reasm_frames as rf

from tests.helpers import build_native_test  # __graft_entry__.build() makes it too


def test_cpp_reasm_compiles_and_links():
    exe = build_native_test("cpp_reasm_test")
    r = subprocess.run([exe, "--link"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["link", "ok", "4", "8"]


@pytest.mark.gpu
def test_cpp_reasm_gpu(engine, tmp_path):
    exe = build_native_test("cpp_reasm_test")
    frames = [f for name, _, fs in rf.cases()[4:] if not name.startswith("mtu 68") for f in fs if f is not None and len(f) < 2100]
    p = tmp_path / "frames.txt"
    p.write_text("".join((f.hex() or "-") + "\n" for f in frames))
    r = subprocess.run([exe, "--gpu", str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    it = iter(l.split() for l in r.stdout.splitlines())
    out, src, rows, _ = reassemble_host(frames, exact=False)
    held = np.flatnonzero(rows["kind"] == abi.REASM_HELD)
    assert len(out) > 100 and len(held) > 20 and (rows["flags"] == abi.REASM_COLLISION).any()
    for align in (1, 16):
        _, offs = pack_host(out, align)
        assert next(it) == ["W", str(align), str(len(frames)), str(len(out)), str(int(offs[-1])), str(len(held))]
        for i, row in enumerate(rows):
            assert next(it) == ["R"] + [str(int(row[n])) for n in abi.REASM_DTYPE.names], (align, i)
        for f, x in enumerate(out):
            assert next(it) == ["F", str(int(offs[f])), str(int(src[f])), x.hex() or "-"], (align, f)
        for i in held:
            assert next(it) == ["H", str(int(i))], (align, i)
    assert next(it, None) is None
