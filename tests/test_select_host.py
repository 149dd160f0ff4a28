"""CPU: the host side of frame selection and gather (nex_amd/select.py).

match_host is the executable statement of nexg_select_batch's contract; the
hand-derived truth table tests/golden/select_cases.json pins it (frame hex,
rule, expected verdict: not reference output, the reference has no filter).
Also: the builders raise ValueError exactly where the C entry returns
NEXG_EINVAL (nexg_filter_check), the struct layouts match the C compiler's,
the library exports the new symbols, gather_host's byte layout, and every rule
the GPU tests run selects some but not all of the corpus."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from nex_amd import abi
from nex_amd import select as S
from nex_amd.select import Filter, Rule
from tests import select_frames as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "nexg.h")
LIB = os.path.join(ROOT, "nex_amd", "libnexg.so")
CASES = os.path.join(ROOT, "tests", "golden", "select_cases.json")

TEST_BITS = {"PROTO": abi.RULE_PROTO, "SRC_PORT": abi.RULE_SRC_PORT, "DST_PORT": abi.RULE_DST_PORT,
             "ANY_PORT": abi.RULE_ANY_PORT, "SRC_ADDR": abi.RULE_SRC_ADDR, "DST_ADDR": abi.RULE_DST_ADDR,
             "ANY_ADDR": abi.RULE_ANY_ADDR, "TCP_FLAGS": abi.RULE_TCP_FLAGS, "LENGTH": abi.RULE_LENGTH}


def rule_from_json(d):
    r = Rule()
    for k, v in d.items():
        if k == "tests":
            for name in v:
                r.tests |= TEST_BITS[name]
        elif k in ("sport", "dport", "len"):
            setattr(r, k + "_lo", v[0])
            setattr(r, k + "_hi", v[1])
        elif k in ("src", "dst"):
            setattr(r, k, sf.ip(v).ljust(16, b"\0"))
        else:
            setattr(r, k, v)
    return r


@pytest.fixture(scope="module")
def table():
    with open(CASES) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def corpus_records(oracle):
    c = sf.corpus()
    return c, oracle.parse_frames([x.frame for x in c], sf.PARSE_FLAGS)


def test_truth_table(oracle, table):
    assert "hand-derived" in " ".join(table["_comment"]).lower()
    frames = {k: bytes.fromhex(v) for k, v in table["frames"].items()}
    recs = {k: oracle.parse_frame(v, table["parse_flags"]) for k, v in frames.items()}
    assert len(table["cases"]) >= 70
    kinds = set()
    for i, c in enumerate(table["cases"]):
        flt = Filter([rule_from_json(r) for r in c["rules"]], invert=c["invert"])
        fr = frames[c["frame"]]
        got = S.match_host(fr, recs[c["frame"]], len(fr), flt)
        assert list(got) == c["expect"], (i, c["frame"], c["why"], got)
        for r in flt.rules:
            kinds.add(r.tests)
    # each test kind alone, pairs, 16 rules and INVERT are all in the table
    assert all(bit in kinds for bit in TEST_BITS.values())
    assert any(bin(k).count("1") >= 2 for k in kinds)
    assert any(len(c["rules"]) == 16 for c in table["cases"]) and any(c["invert"] for c in table["cases"])


def test_junk_field_traps(corpus_records):
    """An error-status frame never matches a port, address, protocol or
    TCP-flag test even when the error payload in its fields would; an ARP
    frame never matches a port or address test."""
    c, recs = corpus_records
    errs = [i for i, x in enumerate(c) if x.status]
    assert sorted(c[i].status for i in errs) == [1, 2, 3, 4]
    arps = [i for i, x in enumerate(c) if x.arp]
    assert arps
    for i in errs + arps:
        r = recs[i]
        if c[i].status:
            assert (int(r["flags"]) >> abi.STATUS_SHIFT) & 7 == c[i].status
        fr, n = c[i].frame, len(c[i].frame)
        a4 = int(r["ip_src"]).to_bytes(4, "big").ljust(16, b"\0")
        d4 = int(r["ip_dst"]).to_bytes(4, "big").ljust(16, b"\0")
        junk = [Rule(tests=abi.RULE_SRC_PORT, sport_lo=int(r["src_port"]), sport_hi=int(r["src_port"])),
                Rule(tests=abi.RULE_DST_PORT, dport_lo=int(r["dst_port"]), dport_hi=int(r["dst_port"])),
                Rule(tests=abi.RULE_ANY_PORT, sport_lo=0, sport_hi=65535),
                Rule(tests=abi.RULE_SRC_ADDR, family=4, src=a4, src_bits=32),
                Rule(tests=abi.RULE_DST_ADDR, family=4, dst=d4, dst_bits=32),
                Rule(tests=abi.RULE_ANY_ADDR, family=4, src_bits=0),
                Rule(tests=abi.RULE_ANY_ADDR, family=6, src_bits=0)]
        if c[i].status:
            junk += [Rule(tests=abi.RULE_PROTO, ip_proto=int(r["ip_proto"])),
                     Rule(tests=abi.RULE_TCP_FLAGS, tcp_mask=0xFF, tcp_value=int(r["l4_type"])),
                     Rule(tests=abi.RULE_TCP_FLAGS, tcp_mask=0, tcp_value=0)]
        for rule in junk:
            assert S.match_host(fr, r, n, Filter([rule])) == (False, abi.RULE_NONE), (c[i].what, rule)
        # while the flags test and the length test still hold for them
        assert S.match_host(fr, r, n, Filter([Rule.length(n)])) == (True, 0)
        assert S.match_host(fr, r, n, Filter([Rule.flags(0xFFFFFFFF, int(r["flags"]))])) == (True, 0)


def test_corpus_classes_match_the_oracle(corpus_records):
    """The classes each corpus frame claims by construction are what the
    parse reports (so the rules' expected picks are meaningful)."""
    c, recs = corpus_records
    assert 55 <= len(c) <= 70
    for x, r in zip(c, recs):
        want = sf.expected_flags(x)
        if want is None:
            continue
        assert int(r["flags"]) == want, (x.what, hex(int(r["flags"])), hex(want))
        if x.l4 in ("tcp", "udp"):
            assert (int(r["src_port"]), int(r["dst_port"])) == (x.sport, x.dport), x.what
        if x.l4 == "tcp":
            assert int(r["l4_type"]) == x.tcp_flags, x.what
        if x.fam == 4:
            assert int(r["ip_src"]).to_bytes(4, "big") == sf.ip(x.src) and int(r["ip_dst"]).to_bytes(4, "big") == sf.ip(x.dst)
        if x.fam == 6:
            l3 = int(r["l3_off"])
            assert x.frame[l3 + 8: l3 + 24] == sf.ip(x.src) and x.frame[l3 + 24: l3 + 40] == sf.ip(x.dst), x.what


def test_every_table_rule_selects_some_but_not_all(corpus_records):
    c, recs = corpus_records
    frames, lens = [x.frame for x in c], [len(x.frame) for x in c]
    for name, rule in sf.RULES.items():
        idx, _ = S.select_host(frames, recs, lens, Filter([rule]))
        assert 0 < len(idx) < len(c), (name, len(idx))
    for name, flt in sf.FILTERS.items():
        idx, rule = S.select_host(frames, recs, lens, flt)
        if name not in ("match all", "match none"):
            assert 0 < len(idx) < len(c), (name, len(idx))
    idx, rule = S.select_host(frames, recs, lens, sf.FILTERS["overlapping"])
    assert len(set(rule.tolist())) >= 3  # first-match order shows in out_rule
    idx, rule = S.select_host(frames, recs, lens, sf.FILTERS["sixteen"])
    assert {14, 15} <= set(rule.tolist())


def test_prefix_bit_frames(corpus_records):
    """X/n picks the frame whose source differs from X at bit k exactly when k > n."""
    c, recs = corpus_records
    by = {x.what: i for i, x in enumerate(c)}
    for n in sf.PREFIX_BITS:
        flt = Filter([Rule.net(f"{sf.X6}/{n}", "src")])
        for k in sf.PREFIX_BITS:
            i = by[f"v6 src X bit {k}"]
            assert S.match_host(c[i].frame, recs[i], len(c[i].frame), flt)[0] == (k > n), (n, k)
        i = by["v6 src X"]
        assert S.match_host(c[i].frame, recs[i], len(c[i].frame), flt)[0]


def test_hostile_record_host(corpus_records):
    """l3_off past the frame, or a frame that is not there, fails the IPv6 tests only."""
    c, recs = corpus_records
    i = next(i for i, x in enumerate(c) if x.what == "v6 udp to 53")
    r = recs[i].copy()
    flt6, fltp = Filter([Rule.net("::/0", "src")]), Filter([Rule.port(53)])
    n = len(c[i].frame)
    assert S.match_host(c[i].frame, r, n, flt6)[0]
    r["l3_off"] = n - 39
    assert not S.match_host(c[i].frame, r, n, flt6)[0] and S.match_host(c[i].frame, r, n, fltp)[0]
    r["l3_off"] = 65535
    assert not S.match_host(c[i].frame, r, n, flt6)[0]
    assert not S.match_host(None, recs[i], n, flt6)[0] and S.match_host(None, recs[i], n, fltp)[0]


# ---- validation: ValueError in Python exactly where C says NEXG_EINVAL -----------

def _bad_rules():
    a = bytes(16)
    return {
        "unknown test bit": Rule(tests=0x200),
        "reserved": Rule(reserved=1),
        "family 0": Rule(tests=abi.RULE_SRC_ADDR, family=0),
        "family 5": Rule(tests=abi.RULE_DST_ADDR, family=5),
        "family 4 any": Rule(tests=abi.RULE_ANY_ADDR, family=7),
        "v4 src_bits 33": Rule(tests=abi.RULE_SRC_ADDR, family=4, src=a, src_bits=33),
        "v4 dst_bits 33": Rule(tests=abi.RULE_DST_ADDR, family=4, dst=a, dst_bits=33),
        "v4 any bits 33": Rule(tests=abi.RULE_ANY_ADDR, family=4, src=a, src_bits=33),
        "v6 src_bits 129": Rule(tests=abi.RULE_SRC_ADDR, family=6, src_bits=129),
        "v6 dst_bits 129": Rule(tests=abi.RULE_DST_ADDR, family=6, dst_bits=129),
        "sport lo > hi": Rule(tests=abi.RULE_SRC_PORT, sport_lo=2, sport_hi=1),
        "any port lo > hi": Rule(tests=abi.RULE_ANY_PORT, sport_lo=2, sport_hi=1),
        "dport lo > hi": Rule(tests=abi.RULE_DST_PORT, dport_lo=2, dport_hi=1),
        "len lo > hi": Rule(tests=abi.RULE_LENGTH, len_lo=2, len_hi=1),
        "any port with src": Rule(tests=abi.RULE_ANY_PORT | abi.RULE_SRC_PORT),
        "any port with dst": Rule(tests=abi.RULE_ANY_PORT | abi.RULE_DST_PORT),
        "any port with dport_lo": Rule(tests=abi.RULE_ANY_PORT, sport_hi=9, dport_lo=1, dport_hi=1),
        "any port with dport_hi": Rule(tests=abi.RULE_ANY_PORT, sport_hi=9, dport_hi=1),
        "any addr with src": Rule(tests=abi.RULE_ANY_ADDR | abi.RULE_SRC_ADDR, family=4),
        "any addr with dst": Rule(tests=abi.RULE_ANY_ADDR | abi.RULE_DST_ADDR, family=6),
        "any addr with dst_bits": Rule(tests=abi.RULE_ANY_ADDR, family=4, dst_bits=1),
    }


def _good_rules():
    return {
        "ranges not under test may be reversed": Rule(sport_lo=2, sport_hi=1, dport_lo=2, dport_hi=1, len_lo=2, len_hi=1),
        "family not under test": Rule(family=9, src_bits=200, dst_bits=200),
        "dst_bits unused by SRC_ADDR": Rule(tests=abi.RULE_SRC_ADDR, family=4, src_bits=32, dst_bits=99),
        "v6 128": Rule(tests=abi.RULE_SRC_ADDR | abi.RULE_DST_ADDR, family=6, src_bits=128, dst_bits=128),
        "everything": Rule(tests=abi.RULE_ALL & ~(abi.RULE_ANY_PORT | abi.RULE_ANY_ADDR), family=4, sport_hi=1, dport_hi=1,
                           len_hi=1),
    }


@pytest.fixture(scope="module")
def clib():
    if not os.path.exists(LIB):
        pytest.fail("nex_amd/libnexg.so is not built")
    lib = ctypes.CDLL(LIB)
    lib.nexg_filter_check.restype = ctypes.c_int
    lib.nexg_filter_check.argtypes = [ctypes.POINTER(abi.FilterC)]
    return lib


def _c_check(clib, flt):
    c = flt.to_c(validate=False)
    return clib.nexg_filter_check(ctypes.byref(c))


def test_validation_python_and_c_agree(clib):
    for name, r in _bad_rules().items():
        with pytest.raises(ValueError):
            r.validate()
        with pytest.raises(ValueError):
            Filter([Rule.any(), r]).to_c()
        assert _c_check(clib, Filter([Rule.any(), r])) == abi.EINVAL, name
    for name, r in _good_rules().items():
        r.validate()
        assert _c_check(clib, Filter([r])) == abi.OK, name
    for name, rule in sf.RULES.items():
        assert _c_check(clib, Filter([rule])) == abi.OK, name
    for name, flt in sf.FILTERS.items():
        assert _c_check(clib, flt) == abi.OK, name
    # the filter itself: n_rules 0 and 17, unknown flag bits, NULL
    for flt in (Filter([]), Filter([Rule.any()], flags=2), Filter([Rule.any()], flags=0x80000001)):
        with pytest.raises(ValueError):
            flt.validate()
        assert _c_check(clib, flt) == abi.EINVAL
    with pytest.raises(ValueError):
        Filter([Rule.any()] * 17).validate()
    c = Filter([Rule.any()]).to_c()
    c.n_rules = 17
    assert clib.nexg_filter_check(ctypes.byref(c)) == abi.EINVAL
    c.n_rules = 16  # the unused rules are zero: match-all rules, valid
    assert clib.nexg_filter_check(ctypes.byref(c)) == abi.OK
    assert clib.nexg_filter_check(None) == abi.EINVAL
    # a rule past n_rules is not looked at
    c = Filter([Rule.any()]).to_c()
    c.rules[1].reserved = 1
    assert clib.nexg_filter_check(ctypes.byref(c)) == abi.OK


def test_builders():
    r = Rule.tcp(syn=True, ack=False) & Rule.net("10.0.0.0/8", "dst")
    assert (r.flags_mask, r.flags_value, r.tests) == (abi.L_TCP, abi.L_TCP, abi.RULE_TCP_FLAGS | abi.RULE_DST_ADDR)
    assert (r.tcp_mask, r.tcp_value, r.family, r.dst_bits, r.dst[:4]) == (0x12, 0x02, 4, 8, bytes([10, 0, 0, 0]))
    r = Rule.host("2001:db8::1")
    assert (r.tests, r.family, r.src_bits, r.src) == (abi.RULE_ANY_ADDR, 6, 128, sf.ip("2001:db8::1"))
    r = Rule.port(53)
    assert (r.tests, r.sport_lo, r.sport_hi, r.dport_lo, r.dport_hi) == (abi.RULE_ANY_PORT, 53, 53, 0, 0)
    r = Rule.port(1000, 2000, "dst")
    assert (r.tests, r.dport_lo, r.dport_hi) == (abi.RULE_DST_PORT, 1000, 2000)
    r = Rule.bad_checksum("ip")
    assert (r.flags_mask, r.flags_value) == (abi.C_IP_CHECKED | abi.C_IP_OK, abi.C_IP_CHECKED)
    r = Rule.status(abi.ERR_MALFORMED)
    assert (r.flags_mask, r.flags_value) == (7 << 24, 3 << 24)
    assert Rule.udp().flags_value == abi.L_UDP
    for bad in (lambda: Rule.port(70000), lambda: Rule.port(5, 4), lambda: Rule.net("10.0.0.0/8", "both"),
                lambda: Rule.status(8), lambda: Rule.bad_checksum("l5"), lambda: Rule.port(1) & Rule.port(2),
                lambda: Rule.net("10.0.0.0/8", "src") & Rule.net("::/0", "dst"),
                lambda: Rule.flags(abi.L_TCP) & Rule.flags(abi.L_TCP, 0)):
        with pytest.raises(ValueError):
            bad()
    c = Filter([Rule.net("2001:db8::/32", "src")], invert=True).to_c()
    assert (c.n_rules, c.flags, bytes(c.rules[0].src)[:4], c.rules[0].src_bits) == (1, 1, bytes([0x20, 1, 0xd, 0xb8]), 32)


def test_struct_layouts_match_c(tmp_path):
    """sizeof 64 and 1032, every offset, and the constants, against the C compiler."""
    rf = [f for f, _ in abi.RuleC._fields_]
    consts = ["NEXG_RULE_PROTO", "NEXG_RULE_SRC_PORT", "NEXG_RULE_DST_PORT", "NEXG_RULE_ANY_PORT", "NEXG_RULE_SRC_ADDR",
              "NEXG_RULE_DST_ADDR", "NEXG_RULE_ANY_ADDR", "NEXG_RULE_TCP_FLAGS", "NEXG_RULE_LENGTH", "NEXG_RULE_ALL",
              "NEXG_FILTER_INVERT", "NEXG_FILTER_MAX_RULES", "NEXG_RULE_NONE", "NEXG_ABI_VERSION"]
    counts = (0, 1, 256, 257, 65536, 65537, 65793, (1 << 32) - 1)
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HDR}"', 'int main(void){',
             'printf("%zu %zu\\n", sizeof(nexg_rule), sizeof(nexg_filter));']
    lines += [f'printf("%zu\\n", offsetof(nexg_rule, {f}));' for f in rf]
    lines += [f'printf("%zu\\n", offsetof(nexg_filter, {f}));' for f in ("n_rules", "flags", "rules")]
    lines += [f'printf("%u\\n", (unsigned)({m}));' for m in consts]
    lines += [f'printf("%llu %llu\\n", (unsigned long long)nexg_select_workspace({n}ull), '
              f'(unsigned long long)nexg_gather_plan_workspace({n}ull));' for n in counts]
    lines.append("return 0;}")
    src = tmp_path / "probe_sel.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe_sel"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    out = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    assert out[:2] == [64, 1032] == [ctypes.sizeof(abi.RuleC), ctypes.sizeof(abi.FilterC)]
    p = 2
    assert out[p:p + len(rf)] == [getattr(abi.RuleC, f).offset for f in rf]
    p += len(rf)
    assert out[p:p + 3] == [abi.FilterC.n_rules.offset, abi.FilterC.flags.offset, abi.FilterC.rules.offset] == [0, 4, 8]
    p += 3
    assert out[p:p + len(consts)] == [abi.RULE_PROTO, abi.RULE_SRC_PORT, abi.RULE_DST_PORT, abi.RULE_ANY_PORT,
                                      abi.RULE_SRC_ADDR, abi.RULE_DST_ADDR, abi.RULE_ANY_ADDR, abi.RULE_TCP_FLAGS,
                                      abi.RULE_LENGTH, abi.RULE_ALL, abi.FILTER_INVERT, abi.FILTER_MAX_RULES,
                                      abi.RULE_NONE, 1]
    p += len(consts)
    for i, n in enumerate(counts):
        assert out[p + 2 * i: p + 2 * i + 2] == [abi.select_workspace(n), abi.gather_plan_workspace(n)], n


def test_library_exports_select_symbols(clib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    want = {"nexg_select_batch", "nexg_gather_plan", "nexg_gather_frames", "nexg_gather_rows", "nexg_filter_check"}
    assert want <= exported, want - exported
    assert want <= set(abi.EXPORTED_SYMBOLS)
    clib.nexg_abi_version.restype = ctypes.c_int
    assert clib.nexg_abi_version() == 1


def test_entry_points_reject_a_null_context(clib):
    """Without a device the entry points still refuse cleanly (no context: NEXG_EINVAL)."""
    for name in ("nexg_select_batch", "nexg_gather_plan", "nexg_gather_frames", "nexg_gather_rows"):
        fn = getattr(clib, name)
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p] * 12
        assert fn(*([None] * 12)) == abi.EINVAL, name


def test_gather_host_layout():
    data = bytes(range(200))
    offs, lens = [3, 50, 50, 190, 199, 0], [5, 0, 17, 10, 2, 70000]
    for align in (1, 4, 8, 16):
        o, ln, out = S.gather_host(data, offs, lens, align)
        assert ln.tolist() == [5, 0, 17, 10, 0, 0]  # 199 + 2 leaves the data; 70000 > 65535
        pad = lambda n: (n + align - 1) // align * align  # noqa: E731
        want = np.cumsum([0] + [pad(n) for n in ln.tolist()])
        assert o.tolist() == want.tolist() and len(out) == want[-1]
        for k in range(len(offs)):
            a, n = int(o[k]), int(ln[k])
            assert out[a: a + n].tobytes() == data[offs[k]: offs[k] + n]
            assert not out[a + n: int(o[k + 1])].any()
    with pytest.raises(ValueError):
        S.gather_host(data, offs, lens, 2)
