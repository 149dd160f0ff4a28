"""CPU: the host contract of the fixed-string match (nex_amd/match.py) and the
corpus of tests/match_frames.py.

match_host is pinned by a hand-written truth table (frames written out here,
rows derived by hand from the text of include/nexg.h), and compared on the
whole corpus with an independent reference in this file: lookahead regular
expressions over the region (`bytes` re.I folds ASCII letters only) plus the
window filter. PatternSet.to_c raises ValueError exactly where
nexg_patterns_check returns NEXG_EINVAL. The corpus conditions are asserted
from the reference alone: a corpus that does not reach an edge shows nothing
about a kernel that is wrong there."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from nex_amd import abi
from nex_amd import match as M
from nex_amd.match import Pattern, PatternSet
from tests import match_frames as mf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nex_amd", "libnexg.so")
HDR = os.path.join(ROOT, "include", "nexg.h")


# ---- the truth table -----------------------------------------------------------------

def rec(off, ln, status=0):
    return {"flags": status << abi.STATUS_SHIFT, "payload_off": off, "payload_len": ln}


#: (what, frame, record, length, set, (mask, first_off, first_pat))
HDRS = bytes(range(0x80, 0x80 + 10))  # ten header bytes that are in no pattern
TABLE = [
    ("starts with, at the region's first byte", HDRS + b"\x16\x03\x01", rec(10, 3), 13,
     PatternSet([Pattern.prefix(b"\x16\x03")]), (1, 10, 0)),
    ("starts with, one byte in", HDRS + b"\x00\x16\x03", rec(10, 3), 13,
     PatternSet([Pattern.prefix(b"\x16\x03")]), M.NO_MATCH),
    ("anywhere, ends on the region's last byte", HDRS + b"..ab", rec(10, 4), 14,
     PatternSet([Pattern(b"ab")]), (1, 12, 0)),
    ("cut by the region's end though the frame goes on", HDRS + b"..ab", rec(10, 3), 14,
     PatternSet([Pattern(b"ab")]), M.NO_MATCH),
    ("begins before payload_off", HDRS[:9] + b"a" + b"b...", rec(10, 4), 14,
     PatternSet([Pattern(b"ab")]), M.NO_MATCH),
    ("... which the whole frame holds", HDRS[:9] + b"a" + b"b...", rec(10, 4), 14,
     PatternSet([Pattern(b"ab")], frame=True), (1, 9, 0)),
    ("the whole frame needs no record", b"xxab", None, 4, PatternSet([Pattern(b"ab")], frame=True), (1, 2, 0)),
    ("two patterns, the higher index first", HDRS + b".late.early"[::-1], rec(10, 11), 21,
     PatternSet([Pattern(b"etal"), Pattern(b"ylrae")]), (3, 10, 1)),
    ("a tie goes to the lowest index", HDRS + b"..tie", rec(10, 5), 15,
     PatternSet([Pattern(b"x"), Pattern(b"tie"), Pattern(b"t"), Pattern(b"ti")]), (0b1110, 12, 1)),
    ("overlapping occurrences, window on the start", HDRS + b"aaaaa", rec(10, 5), 15,
     PatternSet([Pattern(b"aaa", offset=(2, 2)), Pattern(b"aaa", offset=(3, 9))]), (1, 12, 0)),
    ("window: off_hi is included", HDRS + b"...m", rec(10, 4), 14, PatternSet([Pattern(b"m", offset=(0, 3))]), (1, 13, 0)),
    ("window: one short", HDRS + b"...m", rec(10, 4), 14, PatternSet([Pattern(b"m", offset=(0, 2))]), M.NO_MATCH),
    ("window: off_lo is included", HDRS + b"...m", rec(10, 4), 14, PatternSet([Pattern(b"m", offset=(3, 9))]), (1, 13, 0)),
    ("nocase folds letters on both sides", HDRS + b"HoSt:", rec(10, 5), 15,
     PatternSet([Pattern(b"hOsT:", nocase=True), Pattern(b"hOsT:")]), (1, 10, 0)),
    ("nocase leaves @ and ` apart", HDRS + b"`", rec(10, 1), 11, PatternSet([Pattern(b"@", nocase=True)]), M.NO_MATCH),
    ("nocase leaves [ and { apart", HDRS + b"{", rec(10, 1), 11, PatternSet([Pattern(b"[", nocase=True)]), M.NO_MATCH),
    ("nocase folds Z", HDRS + b"z", rec(10, 1), 11, PatternSet([Pattern(b"Z", nocase=True)]), (1, 10, 0)),
    ("nocase folds A", HDRS + b"A", rec(10, 1), 11, PatternSet([Pattern(b"a", nocase=True)]), (1, 10, 0)),
    ("nocase leaves 0xC4 and 0xE4 apart", HDRS + b"\xe4", rec(10, 1), 11,
     PatternSet([Pattern(b"\xc4", nocase=True)]), M.NO_MATCH),
    ("16 bytes, the longest", HDRS + b"0123456789ABCDEF", rec(10, 16), 26,
     PatternSet([Pattern(b"0123456789ABCDEF"), Pattern(b"F")]), (3, 10, 0)),
    ("payload_len 0", HDRS + b"ab", rec(10, 0), 12, PatternSet([Pattern(b"ab")]), M.NO_MATCH),
    ("an error status", HDRS + b"ab", rec(10, 2, status=abi.ERR_TRUNCATED), 12, PatternSet([Pattern(b"ab")]), M.NO_MATCH),
    ("the payload ends exactly at the frame's end", HDRS + b"ab", rec(10, 2), 12, PatternSet([Pattern(b"ab")]), (1, 10, 0)),
    ("the payload ends past the frame", HDRS + b"ab", rec(10, 3), 12, PatternSet([Pattern(b"ab")]), M.NO_MATCH),
    ("a bad extent", None, rec(10, 2), 12, PatternSet([Pattern(b"ab")]), M.NO_MATCH),
    ("a length above 65535", b"ab" * 40000, None, 80000, PatternSet([Pattern(b"ab")], frame=True), M.NO_MATCH),
]


@pytest.mark.parametrize("what,frame,record,length,pset,want", TABLE, ids=[t[0] for t in TABLE])
def test_truth_table(what, frame, record, length, pset, want):
    assert M.match_host(frame, record, length, pset) == want


def test_select_predicate():
    rows = np.zeros(6, abi.MATCH_DTYPE)
    rows["mask"] = [0, 1, 2, 3, 4, 7]
    pick = lambda **k: list(M.match_select_host(rows, **k))  # noqa: E731
    assert pick() == [0, 1, 2, 3, 4, 5]
    assert pick(any=3) == [1, 2, 3, 5]
    assert pick(all=3) == [3, 5]
    assert pick(none=1) == [0, 2, 4]
    assert pick(any=6, none=1) == [2, 4]
    assert pick(any=4, all=1) == [5]
    assert pick(all=8) == []


# ---- the independent reference ---------------------------------------------------------

def reference_row(frame, record, length, pset):
    if frame is None or length > 65535:
        return M.NO_MATCH
    if pset.frame:
        start, n = 0, length
    else:
        status = (int(record["flags"]) >> abi.STATUS_SHIFT) & 7
        start, n = int(record["payload_off"]), int(record["payload_len"])
        if status or n == 0 or start + n > length:
            return M.NO_MATCH
    region = bytes(frame[start: start + n])
    mask, best = 0, None
    for i, p in enumerate(pset.patterns):
        rx = re.compile(b"(?=" + re.escape(bytes(p.data)) + b")", (re.I if p.nocase else 0) | re.S)
        at = [m.start() for m in rx.finditer(region) if p.offset[0] <= m.start() <= p.offset[1]]
        if at:
            mask |= 1 << i
            if best is None or (at[0], i) < best:
                best = (at[0], i)
    return (mask, start + best[0], best[1]) if mask else M.NO_MATCH


def reference_rows(oracle, c):
    recs = c.records(oracle)
    return recs, [reference_row(f, r, len(f), c.pset) for f, r in zip(c.frames, recs)]


@pytest.fixture(scope="module")
def refs(oracle):
    return {c.name: reference_rows(oracle, c) for c in mf.cases()}


def test_match_host_equals_the_reference_on_the_corpus(oracle, refs):
    for c in mf.cases():
        _, rows = mf.expected(oracle, c)
        want = refs[c.name][1]
        got = [(int(r["mask"]), int(r["first_off"]), int(r["first_pat"])) for r in rows]
        bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not bad, (c.name, bad[:5], [got[i] for i in bad[:5]], [want[i] for i in bad[:5]])
        assert (rows["reserved"] == 0).all()


# ---- corpus conditions, from the reference alone ---------------------------------------

def test_sweep_reaches_every_position_and_phase(refs):
    for L in mf.SWEEP_L:
        c = mf.case(f"sweep L={L}")
        recs, rows = refs[c.name]
        offs = 1 + np.concatenate([[0], np.cumsum([len(f) for f in c.frames])])  # helpers.packed_from_byte_1
        phases, whole, cut = set(), 0, 0
        for i, note in enumerate(c.notes["planted"]):
            if note is None:  # a follower: it begins with the bytes its neighbour lacks
                n, q, _ = c.notes["planted"][i - 1]
                assert c.frames[i - 1][mf.PAYLOAD_OFF + q:] + c.frames[i][: L - (n - q)] == mf.ALPHA[:L]
                continue
            n, q, fits = note
            assert int(recs["payload_off"][i]) == mf.PAYLOAD_OFF and int(recs["payload_len"][i]) == n
            assert mf.ALPHA[0] not in c.frames[i][:mf.PAYLOAD_OFF] or L == 1
            if fits:
                assert rows[i] == (1, mf.PAYLOAD_OFF + q, 0), (L, n, q)
                phases.add(int(offs[i] + mf.PAYLOAD_OFF + q) % 16)
                whole += 1
            else:
                assert rows[i] == M.NO_MATCH, (L, n, q)
                cut += 1
        assert phases == set(range(16)), (L, phases)
        assert whole == sum(n - L + 1 for n in mf.SWEEP_N if n >= L)
        assert cut == sum(min(L - 1, n) for n in mf.SWEEP_N)


def test_traps_and_shapes(refs):
    rows = refs["header trap payload"][1]
    frows = refs["header trap frame"][1]
    assert rows[0] == (0b1000, mf.PAYLOAD_OFF, 3)  # only the payload's own "xyz"
    assert frows[0] == (0b1111, 0, 2)              # the frame holds all four; its first six bytes come first
    assert frows[0][0] & 0b0011 == 0b0011 and rows[0][0] & 0b0011 == 0
    assert refs["32 at one position"][1][0] == (0xFFFFFFFF, mf.PAYLOAD_OFF + 2, 0)
    assert refs["higher index earlier"][1][0] == (3, mf.PAYLOAD_OFF + 1, 1)
    assert refs["aaa in aaaaa"][1][0] == (0b011, mf.PAYLOAD_OFF, 0)
    assert refs["16 and 1"][1][0] == (3, mf.PAYLOAD_OFF, 0) and refs["16 and 1"][1][2] == M.NO_MATCH
    assert refs["windows"][1][0] == (0b10010, mf.PAYLOAD_OFF + 21, 1)
    assert refs["windows"][1][2][0] == 0b10100 and refs["windows"][1][3][0] == 0b11000
    nc = refs["nocase"][1]
    assert nc[0][0] == 0b000001 and nc[3][0] == 0b000011 and nc[6][0] == 0b000100 and nc[7][0] == 0
    assert nc[11][0] == 0b001000 and nc[13][0] == 0 and nc[14][0] == 0
    em = refs["empty regions"][1]
    assert [r[0] != 0 for r in em] == [False, True, False, False, False, False, True, False, False]
    big = refs["large"][1]
    assert big[1] == (0b1111, mf.PAYLOAD_OFF, 0) and big[3] == M.NO_MATCH  # the last hit's "!" is the frame's last byte
    assert refs["large frame"][1][1] == (0b11, 0, 0)


def test_fuzz_sets_hit_miss_overlap_and_tie(refs):
    many = ties = frames = 0
    for k in mf.FUZZ_SIZES:
        c = mf.case(f"fuzz {k}")
        recs, rows = refs[c.name]
        assert len(c.pset.patterns) == k and len(c.frames) == mf.FUZZ_FRAMES
        masks = np.array([r[0] for r in rows], np.uint64)
        for p in range(k):
            hit = int(((masks >> np.uint64(p)) & np.uint64(1)).sum())
            assert 0 < hit < len(rows), (k, p, hit, c.pset.patterns[p])
        frames += len(rows)
        many += sum(1 for m in masks if bin(int(m)).count("1") >= 2)
        for f, r, row in zip(c.frames, recs, rows):
            if row[0] == 0:
                continue
            start, n = int(r["payload_off"]), int(r["payload_len"])
            region = f[start: start + n]
            q = row[1] - start
            here = 0
            for p in c.pset.patterns:
                a, b = region[q: q + len(p.data)], bytes(p.data)
                same = a.lower() == b.lower() if p.nocase else a == b
                here += bool(same and len(a) == len(b) and p.offset[0] <= q <= p.offset[1])
            ties += here >= 2
        assert any((int(x["flags"]) >> abi.STATUS_SHIFT) & 7 for x in recs)  # error frames are in
    assert many * 4 >= frames, (many, frames)
    assert ties >= 20, ties


# ---- validation ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def clib():
    if not os.path.exists(LIB):
        pytest.fail("nex_amd/libnexg.so is not built")
    lib = ctypes.CDLL(LIB)
    lib.nexg_patterns_check.restype = ctypes.c_int
    lib.nexg_patterns_check.argtypes = [ctypes.POINTER(abi.PatternsC)]
    return lib


def test_validation_python_and_c_agree(clib):
    for name, s in mf.invalid_sets().items():
        with pytest.raises(ValueError):
            s.to_c()
        c = s.to_c(validate=False)
        assert clib.nexg_patterns_check(ctypes.byref(c)) == abi.EINVAL, name
    valid = [PatternSet([Pattern(b"a")]), PatternSet([Pattern(b"x" * 16, nocase=True, offset=(65535, 65535))] * 32, frame=True),
             PatternSet([Pattern.prefix(b"\x16\x03")])] + [c.pset for c in mf.cases()]
    for s in valid:
        assert clib.nexg_patterns_check(ctypes.byref(s.to_c())) == abi.OK
    assert clib.nexg_patterns_check(None) == abi.EINVAL
    c = PatternSet([Pattern(b"a")]).to_c()
    c.pat[1].len = 99  # a pattern past n_patterns is not looked at
    assert clib.nexg_patterns_check(ctypes.byref(c)) == abi.OK
    c.n_patterns = 2
    assert clib.nexg_patterns_check(ctypes.byref(c)) == abi.EINVAL


def test_struct_layouts_match_c(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HDR}"', 'int main(void){',
             'printf("%zu %zu %zu\\n", sizeof(nexg_pattern), sizeof(nexg_patterns), sizeof(nexg_match));']
    lines += [f'printf("%zu\\n", offsetof(nexg_pattern, {f}));' for f, _ in abi.PatternC._fields_]
    lines += [f'printf("%zu\\n", offsetof(nexg_match, {f}));' for f in abi.MATCH_DTYPE.names]
    lines += [f'printf("%u\\n", (unsigned)({m}));' for m in
              ("NEXG_MATCH_MAX_PATTERNS", "NEXG_MATCH_MAX_LEN", "NEXG_PAT_NOCASE", "NEXG_MATCH_FRAME", "NEXG_PAT_NONE")]
    lines += [f'printf("%llu\\n", (unsigned long long)nexg_match_select_workspace({n}ull));' for n in (0, 1, 65536, 65537)]
    lines.append("return 0;}")
    src = tmp_path / "probe_match.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe_match"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    out = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    assert out[:3] == [ctypes.sizeof(abi.PatternC), ctypes.sizeof(abi.PatternsC), abi.MATCH_DTYPE.itemsize]
    k = 3 + len(abi.PatternC._fields_)
    assert out[3:k] == [getattr(abi.PatternC, f).offset for f, _ in abi.PatternC._fields_]
    assert out[k:k + 4] == [abi.MATCH_DTYPE.fields[f][1] for f in abi.MATCH_DTYPE.names]
    assert out[k + 4:k + 9] == [abi.MATCH_MAX_PATTERNS, abi.MATCH_MAX_LEN, abi.PAT_NOCASE, abi.MATCH_FRAME, abi.PAT_NONE]
    assert out[k + 9:] == [abi.match_select_workspace(n) for n in (0, 1, 65536, 65537)]


def test_library_exports_match_symbols(clib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    want = {"nexg_patterns_check", "nexg_match_batch", "nexg_match_select"}
    assert want <= exported and want <= set(abi.EXPORTED_SYMBOLS)
