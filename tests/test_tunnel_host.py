"""CPU: the host side of tunnel decapsulation. nex_amd.tunnel (decap_host,
tunnel_view, the header views) reproduces the byte vectors the reference's own
unit tests assert (tests/golden/tunnel_vectors.json: vxlan.rs, gre.rs), the
generator of the GPU tests agrees with decap_host, and include/nexg.h,
nex_amd/abi.py and libnexg.so agree on the new structs and entry points."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from nex_amd import abi, tunnel
from oracle import oracle
from tests import tunnel_frames as tf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "nexg.h")
LIB = os.path.join(ROOT, "nex_amd", "libnexg.so")


def _udp_record(n):
    """Record of a frame that is nothing but a UDP payload to the VXLAN port."""
    return {"flags": abi.L_ETHERNET | abi.L_IP | abi.L_IPV4 | abi.L_TRANSPORT | abi.L_UDP, "payload_off": 0,
            "payload_len": n, "dst_port": 4789, "ip_proto": 17}


def _gre_record(n):
    return {"flags": abi.L_ETHERNET | abi.L_IP | abi.L_IPV4, "payload_off": 0, "payload_len": n, "dst_port": 0,
            "ip_proto": 47}


def _check_vector(v, raw, frame, rec, kind):
    t, ioff, ilen = tunnel.decap_host(frame, rec)
    poff = int(rec["payload_off"])
    assert t["kind"] == kind, v["name"]
    if not v["parsed"]:
        assert t["status"] == abi.ERR_MALFORMED and (ioff, ilen) == (0, 0), v["name"]
        assert all(t[n] == 0 for n in ("inner", "hdr_len", "flags", "proto", "id", "aux")), v["name"]
        assert tunnel.tunnel_view(t, frame, rec) is None
        return
    assert t["status"] == abi.FRAME_OK, v["name"]
    assert frame[ioff:ioff + ilen].hex() == v["payload"], v["name"]
    assert ioff == poff + t["hdr_len"] and ilen == len(raw) - t["hdr_len"], v["name"]
    view = tunnel.tunnel_view(t, frame, rec)
    for k, want in v["fields"].items():
        assert getattr(view, k) == want, (v["name"], k, getattr(view, k), want)
    # the tests' round trip: to_bytes() of the parsed packet is the input
    assert view.to_bytes() + frame[ioff:ioff + ilen] == raw, v["name"]
    if kind == abi.TUN_GRE:
        assert t["hdr_len"] == v["header_len"] == view.header_len(), v["name"]
        assert t["proto"] == v["fields"]["protocol_type"]
        assert t["inner"] == tunnel.GRE_INNER.get(t["proto"], abi.INNER_OTHER)
    else:
        assert (t["hdr_len"], t["inner"], t["proto"]) == (8, abi.INNER_ETHERNET, 0), v["name"]
        assert t["id"] == v["fields"]["vni"] and t["flags"] == v["fields"]["flags"]


@pytest.mark.parametrize("wrapped", [False, True])
def test_reference_vectors(wrapped):
    """Every vector, as a bare payload under a synthetic record and wrapped in
    real outer headers under the oracle's record; the routing vector is
    malformed."""
    g = tf.vectors()
    for fam, kind, mk in (("vxlan", abi.TUN_VXLAN, _udp_record), ("gre", abi.TUN_GRE, _gre_record)):
        assert g[fam]
        for v in g[fam]:
            raw = bytes.fromhex(v["bytes"])
            if wrapped:
                frame = tf.outer_udp(raw, 4789, False) if kind == abi.TUN_VXLAN else tf.outer_ip(raw, 47, True)
                rec = oracle.parse_frame(frame)
                assert int(rec["payload_len"]) == len(raw)
            else:
                frame, rec = raw, mk(len(raw))
            _check_vector(v, raw, frame, rec, kind)
    assert [v["name"] for v in g["gre"] if not v["parsed"]] == ["gre_with_routing_present_is_not_parsed"]


def test_gre_to_bytes_vector():
    """gre.rs:355-361: a header with the routing bit serialises checksum,
    offset and the routing bytes."""
    for v in tf.vectors()["gre_to_bytes"]:
        f = dict(v["fields"])
        f["routing"] = bytes.fromhex(f["routing"])
        h = tunnel.GreHeader(**f)
        assert h.to_bytes().hex() == v["header"]
        assert (h.to_bytes() + bytes.fromhex(v["payload"])).hex() == v["bytes"]
        assert h.header_len() == len(bytes.fromhex(v["header"]))


def test_decap_host_rules():
    """The candidate rules of include/nexg.h that no reference vector covers."""
    vh = tf.vxlan_header(0x123456, flags=0, reserved1=0xA1A2A3, reserved2=0x7F)
    t, ioff, ilen = tunnel.decap_host(vh + b"xyz", _udp_record(11))
    assert (t["kind"], t["flags"], t["id"], t["aux"], ioff, ilen) == (abi.TUN_VXLAN, 0, 0x123456, 0xA1A2A37F, 8, 3)
    # another port, a custom port, port 0 = 4789, one kind only
    assert tunnel.decap_host(vh, dict(_udp_record(8), dst_port=4790))[0]["kind"] == abi.TUN_NONE
    assert tunnel.decap_host(vh, dict(_udp_record(8), dst_port=4790), vxlan_port=4790)[0]["kind"] == abi.TUN_VXLAN
    assert tunnel.decap_host(vh, _udp_record(8), vxlan_port=0)[0]["kind"] == abi.TUN_VXLAN
    assert tunnel.decap_host(vh, _udp_record(8), which=abi.DECAP_GRE)[0]["kind"] == abi.TUN_NONE
    g = tf.gre_header(0x6558, c=1, k=1, s=1, key=0xDEADBEEF, seq=7)
    t, ioff, ilen = tunnel.decap_host(g + b"ab", _gre_record(18))
    assert (t["kind"], t["inner"], t["hdr_len"], t["id"], t["aux"], ioff, ilen) == \
        (abi.TUN_GRE, abi.INNER_ETHERNET, 16, 0xDEADBEEF, 7, 16, 2)
    v = tunnel.tunnel_view(t, g + b"ab", _gre_record(18))
    assert (v.checksum, v.offset, v.key, v.sequence) == ([0xC5C5], [0x0FF0], [0xDEADBEEF], [7])
    assert tunnel.decap_host(g, _gre_record(16), which=abi.DECAP_VXLAN)[0]["kind"] == abi.TUN_NONE
    for cut in range(16):  # short of any optional field: malformed
        t, ioff, ilen = tunnel.decap_host(g[:cut], _gre_record(cut))
        assert (t["kind"], t["status"], ioff, ilen) == (abi.TUN_GRE, abi.ERR_MALFORMED, 0, 0), cut
    # a transport / ICMP layer, an error status, a record reaching past the frame: no candidate
    for rec in (dict(_gre_record(16), flags=_gre_record(16)["flags"] | abi.L_ICMP),
                dict(_gre_record(16), flags=abi.ERR_MALFORMED << abi.STATUS_SHIFT), _gre_record(17),
                dict(_gre_record(16), payload_off=1)):
        assert tunnel.decap_host(g, rec) == (tunnel._tun(), 0, 0)


def test_generator_agrees_with_decap_host():
    """Each generated case's implied tunnel kind, status, inner class and
    inner bytes are what decap_host finds under the oracle's record."""
    cases = tf.cases()
    assert {c.kind for c in cases} == {0, 1, 2} and {c.inner_class for c in cases if c.inner is not None} == {0, 1, 2, 3}
    for c in cases:
        rec = oracle.parse_frame(c.frame, abi.PARSE_VLAN)
        t, ioff, ilen = tunnel.decap_host(c.frame, rec)
        assert (t["kind"], t["status"]) == (c.kind, c.status), c.what
        if c.inner is None:
            assert (ioff, ilen) == (0, 0), c.what
        else:
            assert t["inner"] == c.inner_class and c.frame[ioff:ioff + ilen] == c.inner, c.what
        if c.vlan:  # without the VLAN extension the tagged outer frame is no tunnel
            assert tunnel.decap_host(c.frame, oracle.parse_frame(c.frame))[0]["kind"] == abi.TUN_NONE, c.what


def test_tunnel_layouts_match_c(tmp_path):
    names = abi.TUNNEL_DTYPE.names
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HDR}"', 'int main(void){',
             'printf("%zu %zu\\n", sizeof(nexg_tunnel), sizeof(nexg_decap_option));']
    lines += [f'printf("%zu\\n", offsetof(nexg_tunnel, {f}));' for f in names]
    lines += [f'printf("%zu\\n", offsetof(nexg_decap_option, {f}));' for f, _ in abi.DecapOption._fields_]
    lines += [f'printf("%u\\n", (unsigned)({m}));' for m in
              ("NEXG_TUN_NONE", "NEXG_TUN_VXLAN", "NEXG_TUN_GRE", "NEXG_INNER_OTHER", "NEXG_INNER_ETHERNET",
               "NEXG_INNER_IPV4", "NEXG_INNER_IPV6", "NEXG_DECAP_VXLAN", "NEXG_DECAP_GRE")]
    lines += [f'printf("%llu\\n", (unsigned long long)nexg_decap_select_workspace({n}ull));'
              for n in (0, 1, 256, 257, 65536, 65537, 65793, 4294967295)]
    lines.append("return 0;}")
    src = tmp_path / "probe_tunnel.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe_tunnel"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    out = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    assert out[:2] == [16, 8] == [abi.TUNNEL_DTYPE.itemsize, ctypes.sizeof(abi.DecapOption)]
    o = out[2:]
    assert o[:len(names)] == [abi.TUNNEL_DTYPE.fields[f][1] for f in names]
    o = o[len(names):]
    assert o[:3] == [getattr(abi.DecapOption, f).offset for f, _ in abi.DecapOption._fields_]
    assert o[3:12] == [abi.TUN_NONE, abi.TUN_VXLAN, abi.TUN_GRE, abi.INNER_OTHER, abi.INNER_ETHERNET, abi.INNER_IPV4,
                       abi.INNER_IPV6, abi.DECAP_VXLAN, abi.DECAP_GRE]
    counts = (0, 1, 256, 257, 65536, 65537, 65793, 4294967295)
    assert o[12:] == [abi.decap_select_workspace(n) for n in counts]
    for n in counts:  # one u32 counter per 256-frame tile fits
        assert abi.decap_select_workspace(n) >= 4 * ((n + 255) // 256)


def test_header_declares_and_library_exports():
    text = open(HDR).read()
    for fn in ("nexg_decap_batch", "nexg_decap_select"):
        assert re.search(r"^int " + fn + r"\(nexg_ctx\* ctx,", text, re.M), fn
        assert fn in abi.EXPORTED_SYMBOLS
    assert "nexg_decap_select_workspace" in abi.HEADER_INLINE
    assert os.path.exists(LIB), "libnexg.so not built"
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {"nexg_decap_batch", "nexg_decap_select"} <= exported
    from nex_amd import _lib
    lib = _lib.load()
    assert lib.nexg_decap_batch.argtypes is not None and lib.nexg_decap_select.argtypes is not None
