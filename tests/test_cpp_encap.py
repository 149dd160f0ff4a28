"""The C++ host API's tunnel encapsulation (include/nexg.hpp nexg::Tunnel,
nexg::TunnelSet, Engine::encap_plan, encap, encap_bufs;
tests/native/cpp_encap_test.cpp). CPU: the wrappers compile with -Wall -Werror
and link against libnexg.so, and the builders refuse what nexg_tunnels_check
refuses. GPU: four tunnels, the index cycling through them and past the set,
give on a 65-frame batch the bytes, offsets and rows of the Python path."""
import subprocess

import numpy as np
import pytest

from nex_amd import abi
from nex_amd.encap import Tunnel, TunnelSet, encap_host, plan_host
from tests import encap_frames as ef

from tests.helpers import build_native_test  # __graft_entry__.build() makes it too


def test_cpp_encap_compiles_links_and_refuses():
    exe = build_native_test("cpp_encap_test")
    r = subprocess.run([exe, "--link"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["link", "ok", "3", "3", "13"]


def tunnels():
    return TunnelSet([
        Tunnel.vxlan(5001, ef.S4, ef.D4, ef.M_DST, ef.M_SRC, src_port=49152, port_span=16384, udp_csum=True, ttl=64, tos=0xB8,
                     ip_id=0x1234, ip_flags=2),
        Tunnel.vxlan(0xABCDEF, ef.S6, ef.D6, ef.M_DST, ef.M_SRC, src_port=40000, dst_port=8472, ttl=33, tos=0x28,
                     flow_label=0xABCDE),
        Tunnel.gre(ef.S4, ef.D4, ef.M_DST, ef.M_SRC, key=0xA1B2C3D4, seq_base=0xFFFFFFF0, ttl=255),
        Tunnel.gre(ef.S6, ef.D6, ef.M_DST, ef.M_SRC, l3=True, ttl=1, flow_label=7)])


@pytest.mark.gpu
def test_cpp_encap_gpu(engine, oracle, tmp_path):
    from nex_amd.engine import FrameBatch
    from tests import helpers
    exe = build_native_test("cpp_encap_test")
    frames = list(ef.small_inner())[:65]
    index = [abi.TUNNEL_NONE if i % 6 == 5 else i % 6 for i in range(len(frames))]
    p = tmp_path / "frames.txt"
    p.write_text("".join((f.hex() or "-") + "\n" for f in frames))
    r = subprocess.run([exe, "--gpu", str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    # the flow rows as the Python path computes them (default parse option, default flow option)
    batch = FrameBatch.from_frames(frames)
    flows = helpers.to_host(engine.flow(batch, engine.parse(batch, out_kind=abi.OUT_RECORD)), abi.FLOW_DTYPE, len(frames))
    want, rows = encap_host(frames, tunnels(), index, flows)
    # the corpus has few flows: tunnel 0's ports are its base port and at least two others taken from a flow hash
    assert int((rows["status"] == abi.FRAME_OK).sum()) >= 60
    assert len({int(v) for v, t in zip(rows["src_port"], rows["tunnel"]) if t == 0}) >= 3
    it = iter(l.split() for l in r.stdout.splitlines())
    for align in (1, 16):
        offs = plan_host([len(w) for w in want], align)
        assert next(it) == ["W", str(align), str(len(frames)), str(int(offs[-1]))]
        for i, (w, row) in enumerate(zip(want, rows)):
            assert next(it) == ["F", str(int(offs[i])), w.hex() or "-"] + [str(v) for v in ef.row_tuple(row)[:3] + ef.row_tuple(row)[4:]], (align, i)
    assert next(it, None) is None
    # and the Python path itself gives the same on the device
    import torch
    t = torch.tensor(index, dtype=torch.uint8, device="cuda")
    out, drows = engine.encap(batch, tunnels(), t, engine.flow(batch, engine.parse(batch, out_kind=abi.OUT_RECORD)), align=16)
    assert (helpers.to_host(drows, abi.ENCAPPED_DTYPE, len(frames)) == rows).all()
    assert (out.offsets.cpu().numpy() == plan_host([len(w) for w in want], 16)).all()
