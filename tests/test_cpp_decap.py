"""The C++ host API's tunnel decapsulation (include/nexg.hpp Engine::decap,
decap_select, decap_bufs; tests/native/cpp_decap_test.cpp). CPU: the wrappers
compile with -Wall -Werror and link against libnexg.so. GPU: the 65-frame
tunnel batch gives the same nexg_tunnel array, inner offsets / lengths and
selections as the Python path."""
import subprocess

import numpy as np
import pytest

from nex_amd import abi

from tests.helpers import build_native_test  # __graft_entry__.build() makes it too


def test_cpp_decap_compiles_and_links():
    exe = build_native_test("cpp_decap_test")
    r = subprocess.run([exe, "--link"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["link", "ok", "3", str(abi.decap_select_workspace(65793)),
                                str(abi.decap_select_workspace(1))]


@pytest.mark.gpu
def test_cpp_decap_gpu(engine, tmp_path):
    import torch
    from nex_amd.engine import FrameBatch
    from nex_amd.frame import ParseOption
    from tests import tunnel_frames as tf
    exe = build_native_test("cpp_decap_test")
    cs = tf.cycled(tf.cases(), 65)
    frames = [c.frame for c in cs]
    p = tmp_path / "frames.txt"
    p.write_text("".join((f.hex() or "-") + "\n" for f in frames))
    r = subprocess.run([exe, "--gpu", str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    t_lines = [l.split() for l in lines if l.startswith("T ")]
    s_lines = [l.split() for l in lines if l.startswith("S ")]
    assert len(t_lines) == 65 and len(s_lines) == 2

    batch = FrameBatch.from_frames(frames, pad_to=4)  # the layout HostBatch builds
    recs = engine.parse(batch, ParseOption(unwrap_vlan=True), out_kind=abi.OUT_RECORD)
    tunnels, inner = engine.decap(batch, recs)
    torch.cuda.synchronize()
    tun = tunnels.cpu().numpy()[: 65 * 16].view(abi.TUNNEL_DTYPE)
    rel = (inner.offsets - batch.offsets[:65]).cpu().numpy()
    ln = inner.lengths.cpu().numpy()
    assert (tun["kind"] != 0).sum() > 30 and {int(k) for k in tun["kind"]} == {0, 1, 2}
    for i, (_, hx, off, n) in enumerate(t_lines):
        assert bytes.fromhex(hx) == tun[i].tobytes(), (i, cs[i].what)
        assert (int(off), int(n)) == (int(rel[i]), int(ln[i])), (i, cs[i].what)
    for (_, mask, k, *idx), classes in zip(s_lines, ({abi.INNER_ETHERNET}, {abi.INNER_IPV4, abi.INNER_IPV6})):
        pidx, sel = engine.decap_select(tunnels, inner, classes)
        assert int(mask) == sum(1 << c for c in classes) and int(k) == sel.count == len(idx)
        assert [int(x) for x in idx] == [int(x) for x in pidx.cpu().numpy().view(np.uint32)]
