"""The C++ host API's flow rows and flow-affine partition (include/nexg.hpp
nexg::FlowOption, Engine::flow, flow_partition, flow_bufs;
tests/native/cpp_flow_test.cpp). CPU: the wrappers compile with -Wall -Werror
and link against libnexg.so, and the header's workspace helper equals
abi.flow_partition_workspace. GPU: the hash, kind and bucket of every frame of
the small corpus at 8 buckets are flow_host's and partition_host's on the
oracle's records."""
import subprocess

import pytest

from nex_amd import abi
from nex_amd.flow import FlowOption, flows_host, partition_host

from tests.helpers import build_native_test  # __graft_entry__.build() makes it too


def test_cpp_flow_compiles_and_links():
    exe = build_native_test("cpp_flow_test")
    r = subprocess.run([exe, "--link"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["link", "ok", "3", str(abi.FLOW_SYMMETRIC | abi.FLOW_KEY), "7",
                                str(abi.flow_partition_workspace(65793, 8)), str(abi.flow_partition_workspace(65793, 256)),
                                str(abi.flow_partition_workspace(0, 1))]


@pytest.mark.gpu
def test_cpp_flow_gpu(oracle, tmp_path):
    from tests import flow_frames as ff
    exe = build_native_test("cpp_flow_test")
    frames = [x.frame for x in ff.small_corpus()]
    recs = oracle.parse_frames(frames, ff.PARSE_FLAGS)
    p = tmp_path / "frames.txt"
    p.write_text("".join((f.hex() or "-") + "\n" for f in frames))
    r = subprocess.run([exe, "--gpu", str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    it = iter(l.split() for l in r.stdout.splitlines())
    for oi, opt in enumerate((FlowOption(), FlowOption(symmetric=True))):
        want = flows_host(frames, recs, [len(f) for f in frames], opt)
        index, first = partition_host(want["hash"], 8)
        assert next(it) == ["O", str(oi), str(len(frames))]
        for i in range(len(frames)):
            w = want[i]
            assert next(it) == ["R", f"{int(w['hash']):08x}", str(w["kind"]), str(w["proto"]), str(w["swapped"]),
                                str(int(w["hash"]) % 8)], (oi, i)
        assert next(it) == ["I"] + [str(i) for i in index], oi
        assert next(it) == ["B"] + [str(b) for b in first], oi
    assert next(it, None) is None
