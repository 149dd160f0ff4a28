"""CPU: the contract of nexg_encap_plan / nexg_encap_frames (include/nexg.h) as
nex_amd.encap.encap_host states it, pinned by an independent reference (the
oracle's Eth / IP / UDP builders around `VXLAN header + inner`, GRE assembled
in tests/encap_frames.py), a hand-written status table, the FLOW_PORT and
sequence arithmetic, a UDP checksum that computes to 0, the round trip through
the oracle's parser and decap_host, nexg_tunnels_check's rejections one by
one, and the struct layouts against a probe compiled from include/nexg.h."""
import ctypes
import os
import subprocess
from dataclasses import replace

import numpy as np
import pytest

from nex_amd import abi
from nex_amd.encap import Tunnel, TunnelSet, encap_frame, encap_host, plan_host
from nex_amd.tunnel import decap_host
from tests import encap_frames as ef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "nexg.h")


def equal(got, want, what):
    (gf, gr), (wf, wr) = got, want
    assert len(gf) == len(wf)
    for i, (a, b) in enumerate(zip(gf, wf)):
        assert a == b, (what, i, len(a), len(b), a[:80].hex(), b[:80].hex())
        assert ef.row_tuple(gr[i]) == ef.row_tuple(wr[i]), (what, i, gr[i], wr[i])


def test_header_lengths():
    want = [50] * 4 + [70] * 4 + [38, 38, 42, 42, 42, 42, 46, 46] + [58, 58, 62, 62, 62, 62, 66, 66]
    assert [t.header_len() for t in ef.specs()] == want
    assert len({(t.kind, t.family, t.flags) for t in ef.specs()}) == 24


def test_host_equals_the_reference_for_every_spec(oracle):
    inner = list(ef.small_inner())
    hashes = ef.hashes_for(len(inner))
    oks = 0
    for tunnels, numbers in ef.spec_sets():
        for j, k in enumerate(numbers):
            frames = inner + ef.limit_inner(ef.specs()[k])
            h = np.concatenate([hashes, [3, 4]]).astype(np.uint32)
            index = [j] * len(frames)
            got = encap_host(frames, tunnels, index, ef.flows_array(h))
            equal(got, ef.ref_all(oracle, frames, tunnels, index, h), f"spec {k}")
            assert got[1]["status"][-2] == abi.FRAME_OK and len(got[0][-2]) == 65535
            assert got[1]["status"][-1] == abi.ERR_INVALID_LENGTH and got[0][-1] == b""
            oks += int((got[1]["status"] == abi.FRAME_OK).sum())
    assert oks > 24 * 70


def test_status_table():
    vx4, vx6 = ef.specs()[0], ef.specs()[4]
    g4, g4l3, g6ksl3 = ef.specs()[8], ef.specs()[9], ef.specs()[23]
    assert g4l3.l3_mode and not g4.l3_mode and g6ksl3.header_len() == 66
    eth = bytes(range(1, 13)) + b"\x88\xb5"
    T = abi
    table = [  # spec, inner, tunnel number, (status, tunnel, hdr_len), output length
        (vx4, b"", 0, (T.FRAME_OK, 0, 50), 50),
        (vx4, bytes(65485), 3, (T.FRAME_OK, 3, 50), 65535),
        (vx4, bytes(65486), 3, (T.ERR_INVALID_LENGTH, 3, 0), 0),
        (vx6, bytes(65465), 1, (T.FRAME_OK, 1, 70), 65535),
        (vx6, bytes(65466), 1, (T.ERR_INVALID_LENGTH, 1, 0), 0),
        (g4, b"", 2, (T.FRAME_OK, 2, 38), 38),
        (g4, bytes(13), 2, (T.FRAME_OK, 2, 38), 51),
        (g4l3, b"", 5, (T.ERR_BUFFER_TOO_SHORT, 5, 0), 0),
        (g4l3, bytes(13), 5, (T.ERR_BUFFER_TOO_SHORT, 5, 0), 0),
        (g4l3, eth, 5, (T.FRAME_OK, 5, 38), 38),
        (g4l3, eth + bytes(65535 - 38), 5, (T.FRAME_OK, 5, 38), 65535),   # a 65511-B frame fits once its header is dropped
        (g4l3, eth + bytes(65535 - 37), 5, (T.ERR_INVALID_LENGTH, 5, 0), 0),
        (g6ksl3, eth + bytes(65535 - 66), 15, (T.FRAME_OK, 15, 66), 65535),
        (g6ksl3, eth + bytes(65535 - 65), 15, (T.ERR_INVALID_LENGTH, 15, 0), 0),
        (None, bytes(65535), 16, (T.FRAME_OK, T.TUNNEL_NONE, 0), 65535),
        (None, b"", 0xFF, (T.FRAME_OK, T.TUNNEL_NONE, 0), 0),
    ]
    for n, (t, inner, number, row, out_len) in enumerate(table):
        out, got = encap_frame(inner, t, 0, 0, number)
        assert got[:3] == row and len(out) == out_len, (n, got, len(out))
    out, got = encap_frame(None, vx4, 0, 0, 77)  # the extent is judged before the index
    assert out == b"" and got == (T.ERR_BAD_EXTENT, 77, 0, 0, 0, 0)
    out, got = encap_frame(eth + b"\x01\x02", g4l3, 0, 0, 5)
    assert out[34:38] == b"\x00\x00\x88\xb5" and out[38:] == b"\x01\x02"  # protocol_type: whatever bytes 12..13 hold


def test_pass_through_and_out_of_range_indices(oracle):
    inner = list(ef.small_inner())[:40]
    tunnels = TunnelSet(ef.specs()[:3])
    index = [(0, 1, 2, 3, abi.TUNNEL_NONE, 16, 77, 200)[i % 8] for i in range(len(inner))]
    frames = [None if i % 11 == 10 else f for i, f in enumerate(inner)]
    got = encap_host(frames, tunnels, index, ef.flows_array(ef.hashes_for(len(inner))))
    equal(got, ef.ref_all(oracle, frames, tunnels, index, ef.hashes_for(len(inner))), "mixed index")
    out, rows = got
    for i, f in enumerate(frames):
        if f is None:
            assert ef.row_tuple(rows[i]) == (abi.ERR_BAD_EXTENT, index[i], 0, 0, 0, 0) and out[i] == b""
        elif index[i] >= 3:
            assert ef.row_tuple(rows[i]) == (0, abi.TUNNEL_NONE, 0, 0, 0, 0) and out[i] == f
    # no index: tunnel 0 for every frame
    plain = TunnelSet([ef.specs()[2], ef.specs()[8]])
    equal(encap_host(inner, plain), ef.ref_all(oracle, inner, plain), "no index")
    with pytest.raises(ValueError):
        encap_host(inner, TunnelSet(ef.specs()[1:2]))  # FLOW_PORT without flows


def test_flow_port_arithmetic(oracle):
    t = Tunnel.vxlan(vni=9, src=ef.S4, dst=ef.D4, src_port=60000, port_span=5536, udp_csum=True)
    inner = ef.small_inner()[16]
    span = 5536
    for h, port in ((0, 60000), (span - 1, 65535), (span, 60000), (span + 1, 60001), (0xFFFFFFFF, 60000 + 0xFFFFFFFF % span)):
        out, row = encap_frame(inner, t, 0, h, 0)
        assert row[4] == port and int.from_bytes(out[34:36], "big") == port
        assert (out, row) == ef.ref_frame(oracle, inner, t, 0, h, 0)
    one = replace(t, port_span=1)
    assert encap_frame(inner, one, 0, 0xDEADBEEF, 0)[1][4] == 60000
    fixed = replace(t, port_span=0, flags=abi.ENCAP_UDP_CSUM)
    assert encap_frame(inner, fixed, 0, 0xDEADBEEF, 0)[1][4] == 60000


def test_sequence_wraps(oracle):
    t = Tunnel.gre(src=ef.S4, dst=ef.D4, key=1, seq_base=0xFFFFFFFE)
    inner = [ef.small_inner()[16]] * 4
    out, rows = encap_host(inner, TunnelSet([t]))
    assert [int.from_bytes(o[42:46], "big") for o in out] == [0xFFFFFFFE, 0xFFFFFFFF, 0, 1]
    equal((out, rows), ef.ref_all(oracle, inner, TunnelSet([t])), "sequence")


def test_a_udp_checksum_of_zero_stays_zero(oracle):
    """No 0 -> 0xFFFF mapping: the source port that makes the
    sum fold to 0xFFFF is found by search, and the field reads 0000."""
    inner = ef.small_inner()[16]
    base = Tunnel.vxlan(vni=77, src=ef.S4, dst=ef.D4, src_port=0, udp_csum=True)
    c0 = encap_frame(inner, base, 0, 0, 0)[1][5]
    port = next(p for p in range(65536) if encap_frame(inner, replace(base, src_port=p), 0, 0, 0)[1][5] == 0)
    t = replace(base, src_port=port)
    out, row = encap_frame(inner, t, 0, 0, 0)
    assert c0 != 0 and row[5] == 0 and out[40:42] == b"\x00\x00"
    assert (out, row) == ef.ref_frame(oracle, inner, t, 0, 0, 0)
    rec = oracle.parse_frame(out)
    assert rec["flags"] & abi.L_UDP and int(rec["src_port"]) == port


def test_round_trip_through_parse_and_decap(oracle):
    inner = list(ef.small_inner())
    for tunnels, numbers in ef.spec_sets():
        for j, k in enumerate(numbers):
            t = ef.specs()[k]
            out, rows = encap_host(inner, tunnels, [j] * len(inner), ef.flows_array(ef.hashes_for(len(inner))))
            for i, (o, f) in enumerate(zip(out, inner)):
                if rows[i]["status"] != abi.FRAME_OK:
                    continue
                rec = oracle.parse_frame(o)
                port = t.dst_port or abi.VXLAN_PORT
                tun, off, n = decap_host(o, rec, vxlan_port=port)
                assert tun["status"] == abi.FRAME_OK and tun["kind"] == t.kind, (k, i, tun)
                assert o[off:off + n] == (f[14:] if t.l3_mode else f), (k, i)
                assert tun["hdr_len"] == t.header_len() - 14 - (20 if t.family == 4 else 40) - (8 if t.kind == abi.ENCAP_VXLAN else 0)
                if t.family == 4:
                    assert rec["flags"] & abi.C_IP_OK, (k, i)
                if t.flags & abi.ENCAP_UDP_CSUM:
                    assert rec["flags"] & abi.C_L4_OK, (k, i)
                if t.kind == abi.ENCAP_VXLAN or t.flags & abi.ENCAP_GRE_KEY:
                    assert tun["id"] == t.id


def test_plan_host():
    assert list(plan_host([50, 0, 51, 16], 1)) == [0, 50, 50, 101, 117]
    assert list(plan_host([50, 0, 51, 16], 16)) == [0, 64, 64, 128, 144]
    assert list(plan_host([], 8)) == [0]


def invalid_sets():
    """name -> nexg_tunnels (ctypes) that nexg_tunnels_check refuses, one reason each."""
    vx, gre = ef.specs()[0], ef.specs()[8]
    flow = ef.specs()[1]

    def one(t):
        return TunnelSet([vx, t]).to_c(check=False)

    out = {
        "kind 0": one(replace(vx, kind=0)), "kind 3": one(replace(vx, kind=3)),
        "family 0": one(replace(vx, family=0)), "family 5": one(replace(gre, family=5)),
        "unknown flag": one(replace(vx, flags=0x20)), "unknown high flag": one(replace(gre, flags=0x80000000)),
        "GRE_KEY on VXLAN": one(replace(vx, flags=abi.ENCAP_GRE_KEY)), "GRE_SEQ on VXLAN": one(replace(vx, flags=abi.ENCAP_GRE_SEQ)),
        "GRE_L3 on VXLAN": one(replace(vx, flags=abi.ENCAP_GRE_L3)), "UDP_CSUM on GRE": one(replace(gre, flags=abi.ENCAP_UDP_CSUM)),
        "FLOW_PORT on GRE": one(replace(gre, flags=abi.ENCAP_FLOW_PORT, port_span=1)),
        "vni 2^24": one(replace(vx, id=1 << 24)), "flow_label 2^20": one(replace(gre, flow_label=1 << 20)),
        "ip_flags 8": one(replace(vx, ip_flags=8)),
        "FLOW_PORT span 0": one(replace(flow, port_span=0)),
        "FLOW_PORT past 65536": one(replace(flow, src_port=65535, port_span=2)),
        "span without FLOW_PORT": one(replace(vx, port_span=1)),
        "reserved[0]": one(replace(vx, reserved=b"\x01" + bytes(22))), "reserved[22]": one(replace(gre, reserved=bytes(22) + b"\x01")),
    }
    empty = TunnelSet([vx]).to_c()
    empty.n_tunnels = 0
    many = TunnelSet([vx] * 16).to_c()
    many.n_tunnels = 17
    res = TunnelSet([vx]).to_c()
    res.reserved = 1
    out.update({"n_tunnels 0": empty, "n_tunnels 17": many, "set reserved": res})
    return out


def test_tunnels_check_rejects_each_case():
    from nex_amd._lib import load
    lib = load()
    for tunnels, _ in ef.spec_sets():
        assert lib.nexg_tunnels_check(ctypes.byref(tunnels.to_c())) == abi.OK
    edge = TunnelSet([Tunnel.vxlan(vni=0xFFFFFF, src=ef.S4, dst=ef.D4, src_port=65535, port_span=1),
                      Tunnel.gre(src=ef.S6, dst=ef.D6, key=0xFFFFFFFF, seq_base=0xFFFFFFFF, flow_label=0xFFFFF, ip_flags=7)])
    assert lib.nexg_tunnels_check(ctypes.byref(edge.to_c())) == abi.OK
    for name, c in invalid_sets().items():
        assert lib.nexg_tunnels_check(ctypes.byref(c)) == abi.EINVAL, name
    assert lib.nexg_tunnels_check(None) == abi.EINVAL
    # the Python builders refuse the same sets
    vx = ef.specs()[0]
    for bad in (replace(vx, kind=3), replace(vx, family=5), replace(vx, flags=0x20), replace(vx, flags=abi.ENCAP_GRE_L3),
                replace(vx, id=1 << 24), replace(vx, flow_label=1 << 20), replace(vx, ip_flags=8), replace(vx, port_span=1),
                replace(ef.specs()[1], port_span=0), replace(vx, reserved=b"\x01" + bytes(22))):
        with pytest.raises(ValueError):
            TunnelSet([bad]).to_c()
    for bad in (TunnelSet([]), TunnelSet([vx] * 17), TunnelSet([vx], reserved=1)):
        with pytest.raises(ValueError):
            bad.to_c()


def test_struct_layouts_match_c(tmp_path):
    spec = [f for f, _ in abi.TunnelSpecC._fields_]
    rows = abi.ENCAPPED_DTYPE.names
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HDR}"', 'int main(void){',
             'printf("%zu %zu %zu %zu\\n", sizeof(nexg_tunnel_spec), sizeof(nexg_tunnels), sizeof(nexg_encapped), '
             'offsetof(nexg_tunnels, tunnels));']
    lines += [f'printf("%zu\\n", offsetof(nexg_tunnel_spec, {f}));' for f in spec]
    lines += [f'printf("%zu\\n", offsetof(nexg_encapped, {f}));' for f in rows]
    lines += [f'printf("%u\\n", (unsigned)({m}));' for m in
              ("NEXG_ENCAP_VXLAN", "NEXG_ENCAP_GRE", "NEXG_ENCAP_UDP_CSUM", "NEXG_ENCAP_FLOW_PORT", "NEXG_ENCAP_GRE_KEY",
               "NEXG_ENCAP_GRE_SEQ", "NEXG_ENCAP_GRE_L3", "NEXG_ENCAP_MAX_TUNNELS", "NEXG_TUNNEL_NONE")]
    lines += ['printf("%llu %llu\\n", (unsigned long long)nexg_encap_plan_workspace(0), '
              '(unsigned long long)nexg_encap_plan_workspace(65793));', "return 0;}"]
    src = tmp_path / "probe_encap.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe_encap"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-o", str(exe), str(src)])
    out = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    assert out[:4] == [96, ctypes.sizeof(abi.TunnelsC), abi.ENCAPPED_DTYPE.itemsize, abi.TunnelsC.tunnels.offset]
    assert out[4:4 + len(spec)] == [getattr(abi.TunnelSpecC, f).offset for f in spec]
    n = 4 + len(spec)
    assert out[n:n + len(rows)] == [abi.ENCAPPED_DTYPE.fields[f][1] for f in rows]
    n += len(rows)
    assert out[n:n + 9] == [abi.ENCAP_VXLAN, abi.ENCAP_GRE, abi.ENCAP_UDP_CSUM, abi.ENCAP_FLOW_PORT, abi.ENCAP_GRE_KEY,
                            abi.ENCAP_GRE_SEQ, abi.ENCAP_GRE_L3, abi.ENCAP_MAX_TUNNELS, abi.TUNNEL_NONE]
    assert out[n + 9:] == [abi.encap_plan_workspace(0), abi.encap_plan_workspace(65793)]
