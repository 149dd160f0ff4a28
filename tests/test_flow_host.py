"""CPU: the host statement of the flow contract (nex_amd/flow.py toeplitz,
flow_host, partition_host) against the published RSS verification vectors
(tests/golden/flow_vectors.json) and a hand-written truth table, on the
oracle's records of the corpus of tests/flow_frames.py; and the ABI mirrors of
the new structs."""
import ctypes
import ipaddress
import os
import subprocess

import numpy as np
import pytest

from nex_amd import abi
from nex_amd import flow as FL
from nex_amd.flow import DEFAULT_KEY, FlowOption, flow_host, partition_host, toeplitz
from tests import flow_frames as ff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER_KEY = bytes((37 * i + 11) & 0xFF for i in range(40))


@pytest.fixture(scope="module")
def corp(oracle):
    items = ff.corpus()
    frames = [x.frame for x in items]
    return items, frames, oracle.parse_frames(frames, ff.PARSE_FLAGS)


def rows(corp, option=FlowOption()):
    items, frames, recs = corp
    return [flow_host(f, r, len(f), option) for f, r in zip(frames, recs)]


def test_toeplitz_golden_vectors():
    vs = ff.vectors()
    assert len(vs) == 8
    for v in vs:
        a = ipaddress.ip_address(v["src"]).packed + ipaddress.ip_address(v["dst"]).packed
        assert toeplitz(a) == v["hash_ip"], v
        assert toeplitz(a + v["sport"].to_bytes(2, "big") + v["dport"].to_bytes(2, "big")) == v["hash_l4"], v
    # linear over GF(2), and a single set bit reads the key window at its position
    assert toeplitz(bytes(36)) == 0
    assert toeplitz(b"\x80") == int.from_bytes(DEFAULT_KEY[:4], "big")
    assert toeplitz(b"\x00\x01") == int.from_bytes(DEFAULT_KEY[:8], "big") >> 17 & 0xFFFFFFFF
    x, y = bytes(range(36)), bytes(range(100, 136))
    assert toeplitz(bytes(a ^ b for a, b in zip(x, y))) == toeplitz(x) ^ toeplitz(y)
    with pytest.raises(ValueError):
        toeplitz(bytes(37))


def test_flow_host_reproduces_golden_on_oracle_records(corp):
    items = corp[0]
    got = rows(corp)
    got_ip = rows(corp, FlowOption(ports=False))
    n = 0
    for x, g, gi in zip(items, got, got_ip):
        if x.hash_l4 is not None:
            assert g[0] == x.hash_l4 and gi[0] == x.hash_ip, x.what
            assert g[1] in (abi.FLOW_IPV4_L4, abi.FLOW_IPV6_L4) and gi[1] in (abi.FLOW_IPV4, abi.FLOW_IPV6)
            n += 1
    assert n == 16  # the eight vectors as TCP and as UDP


def test_truth_table(corp):
    """kind, proto, ports and fragments as the frames' construction implies."""
    items, frames, recs = corp
    got, got_ip = rows(corp), rows(corp, FlowOption(ports=False))
    seen = set()
    for x, f, r, g, gi in zip(items, frames, recs, got, got_ip):
        if x.kind is None:
            continue
        seen.add(x.kind)
        if x.kind == abi.FLOW_NONE:
            assert g == (0, 0, 0, 0) and gi == (0, 0, 0, 0), x.what
            continue
        assert g == (toeplitz(x.key), x.kind, x.proto, 0), x.what
        plain = abi.FLOW_IPV6 if x.kind >= abi.FLOW_IPV6 else abi.FLOW_IPV4
        assert gi == (toeplitz(x.key_ip), plain, x.proto, 0), x.what
        assert len(x.key) == {abi.FLOW_IPV4: 8, abi.FLOW_IPV4_L4: 12, abi.FLOW_IPV6: 32, abi.FLOW_IPV6_L4: 36}[x.kind]
        assert FL.flow_key(f, r, len(f))[3] == x.key, x.what
    assert seen == {0, 1, 2, 3, 4}
    by = {x.what: g for x, g in zip(items, got)}
    assert by["v4 first fragment (MF)"] == by["v4 later fragment (offset 3)"] == by["v4 middle fragment (MF, offset 3)"]
    assert by["5-tuple payload 1"] == by["5-tuple payload 2"] == by["vlan 5-tuple"]
    assert by["vector 0 tcp"][0] == by["vector 0 udp"][0] and by["vector 0 tcp"][2] != by["vector 0 udp"][2]


def test_hostile_record_fields(corp):
    """Only the record decides: an l3_off past the frame, a missing extent and
    an error status give the all-zero row; NEXG_L_IPV4 wins over NEXG_L_IPV6."""
    items, frames, recs = corp
    i = next(k for k, x in enumerate(items) if x.what == "vector 5 tcp")
    f, r = frames[i], recs[i].copy()
    assert flow_host(f, r, len(f))[1] == abi.FLOW_IPV6_L4
    assert flow_host(None, r, len(f)) == (0, 0, 0, 0)
    assert flow_host(f, r, 70000) == (0, 0, 0, 0)
    r["l3_off"] = len(f) - 39
    assert flow_host(f, r, len(f)) == (0, 0, 0, 0)
    r["l3_off"] = len(f) - 40
    assert flow_host(f, r, len(f))[1] == abi.FLOW_IPV6_L4
    r["flags"] = int(r["flags"]) | abi.L_IPV4
    assert flow_host(f, r, len(f))[1] == abi.FLOW_IPV4_L4
    r["flags"] = int(r["flags"]) | (abi.ERR_MALFORMED << abi.STATUS_SHIFT)
    assert flow_host(f, r, len(f)) == (0, 0, 0, 0)


def test_symmetric(corp):
    items = corp[0]
    plain, sym = rows(corp), rows(corp, FlowOption(symmetric=True))
    convs = {}
    for x, p, s in zip(items, plain, sym):
        assert s[1:3] == p[1:3], x.what
        if not s[3]:
            assert s == p, x.what  # not exchanged: the row is the plain one
        if x.conv:
            convs.setdefault(x.conv, []).append((x, p, s))
    assert len(convs) >= 18
    for tag, members in convs.items():
        assert len({s[0] for _, _, s in members}) == 1, tag  # one hash per conversation
    for tag in [f"v{i}{l4}" for i in range(8) for l4 in ("tcp", "udp")] + ["same"]:
        (xa, pa, sa), (xb, pb, sb) = convs[tag]
        assert sa[3] + sb[3] == 1, tag  # exactly one direction was exchanged
        assert (pb if sa[3] else pa)[0] == sa[0], tag  # ... into the other's key
    by = {x.what: s for x, s in zip(items, sym)}
    assert by["same address, ports 9 -> 7"][3] == 1 and by["same address, ports 7 -> 9"][3] == 0
    assert by["same endpoint"][3] == 0
    assert by["arp"] == (0, 0, 0, 0)
    # the vectors: the smaller endpoint first
    for i, v in enumerate(ff.vectors()):
        a, b = ipaddress.ip_address(v["src"]).packed, ipaddress.ip_address(v["dst"]).packed
        assert by[f"vector {i} tcp"][3] == (1 if a > b else 0), i
    # without ports only the addresses are compared
    np_sym = rows(corp, FlowOption(symmetric=True, ports=False))
    by = {x.what: s for x, s in zip(items, np_sym)}
    assert by["same address, ports 9 -> 7"][3] == 0 and by["same address, ports 7 -> 9"][3] == 0


def test_no_ports_and_custom_key(corp):
    items, frames, recs = corp
    ip_only = rows(corp, FlowOption(ports=False))
    keyed = rows(corp, FlowOption(key=OTHER_KEY))
    plain = rows(corp)
    changed = 0
    for x, f, r, gi, gk, gp in zip(items, frames, recs, ip_only, keyed, plain):
        kind, proto, sw, key = FL.flow_key(f, r, len(f))
        assert gk == ((toeplitz(key, OTHER_KEY), kind, proto, sw) if kind else (0, 0, 0, 0)), x.what
        assert gi[1] in (abi.FLOW_NONE, abi.FLOW_IPV4, abi.FLOW_IPV6), x.what
        changed += gk[0] != gp[0]
        if x.hash_ip is not None:
            assert gi[0] == x.hash_ip
    assert changed > len(items) // 2
    # NEXG_FLOW_KEY clear: the key field is ignored
    assert FlowOption(key=OTHER_KEY, flags=0).the_key() == DEFAULT_KEY


def test_option_validation():
    for bad in (FlowOption(flags=0x8), FlowOption(reserved=1), FlowOption(key=bytes(39))):
        with pytest.raises(ValueError):
            bad.to_c()
    c = FlowOption(symmetric=True, ports=False, key=OTHER_KEY).to_c()
    assert c.flags == 7 and c.reserved == 0 and bytes(c.key) == OTHER_KEY
    assert FlowOption().to_c().flags == 0


def test_partition_host_is_stable_and_complete():
    rng = np.random.default_rng(7)
    h = rng.integers(0, 1 << 32, 5000, dtype=np.uint64).astype(np.uint32)
    h[::7] = 0
    for buckets in (1, 2, 3, 8, 255, 256):
        index, first = partition_host(h, buckets)
        assert sorted(index.tolist()) == list(range(len(h)))
        assert first[0] == 0 and first[-1] == len(h) and len(first) == buckets + 1
        for b in range(buckets):
            part = index[first[b]: first[b + 1]]
            assert (h[part].astype(np.int64) % buckets == b).all()
            assert (np.diff(part.astype(np.int64)) > 0).all()
    index, first = partition_host(np.zeros(0, np.uint32), 4)
    assert len(index) == 0 and first.tolist() == [0] * 5
    for bad in (0, 257):
        with pytest.raises(ValueError):
            partition_host(h, bad)


def test_flow_structs_match_c(tmp_path):
    hdr = os.path.join(ROOT, "include", "nexg.h")
    src = tmp_path / "probe.c"
    fields = "".join(f'printf("%zu\\n", offsetof(nexg_flow, {n}));' for n in abi.FLOW_DTYPE.names)
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{hdr}"\nint main(void){{'
                   'printf("%zu %zu %zu %u\\n", sizeof(nexg_flow), sizeof(nexg_flow_option), '
                   'offsetof(nexg_flow_option, key), NEXG_FLOW_TILE);'
                   'static const unsigned char k[40] = NEXG_FLOW_DEFAULT_KEY; for (int i = 0; i < 40; i++) printf("%02x", k[i]);'
                   'printf("\\n");'
                   f'{fields}'
                   'printf("%llu %llu %llu\\n", (unsigned long long)nexg_flow_partition_workspace(0, 8), '
                   '(unsigned long long)nexg_flow_partition_workspace(65793, 256), '
                   '(unsigned long long)nexg_flow_partition_workspace(16777216, 255));return 0;}')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split()
    assert list(map(int, out[:4])) == [8, ctypes.sizeof(abi.FlowOptionC), abi.FlowOptionC.key.offset, abi.FLOW_TILE]
    assert abi.FLOW_DTYPE.itemsize == 8 and ctypes.sizeof(abi.FlowOptionC) == 48
    assert out[4] == DEFAULT_KEY.hex()
    assert list(map(int, out[5:9])) == [abi.FLOW_DTYPE.fields[n][1] for n in abi.FLOW_DTYPE.names[:4]]
    ws = list(map(int, out[5 + len(abi.FLOW_DTYPE.names):]))
    assert ws == [abi.flow_partition_workspace(0, 8), abi.flow_partition_workspace(65793, 256),
                  abi.flow_partition_workspace(16777216, 255)]
    # the issue's ceiling: 4 * buckets * ceil(count / 256) bytes plus a constant
    for count in (0, 1, 255, 1024, 1025, 65793, 1 << 24):
        for buckets in (1, 3, 256):
            assert abi.flow_partition_workspace(count, buckets) <= 4 * buckets * ((count + 255) // 256) + 2048
