"""CPU: nex_amd.reassemble.reassemble_host, the plain-Python statement of
include/nexg.h's reassembly rule that the device output is tested against,
pinned from outside: fragment -> shuffle -> reassemble is the identity, the
oracle parses every output to the record of the original, the truth table of
the completeness rules, the pinned hash collision, and an independent
reference written here (sorted() and bytearray slices; it shares no code with
nex_amd.reassemble)."""
import random

import numpy as np
import pytest

from nex_amd import abi
from nex_amd.flow import toeplitz
from nex_amd.fragment import fragment_host
from nex_amd.reassemble import classify_frame, datagram_complete, key_hash, pack_host, reassemble_host
from tests import fragment_frames as ff
from tests import reasm_frames as rf


# ---- the independent reference -----------------------------------------------------------

def ones_sum(b):
    s = sum(int.from_bytes(b[i:i + 2], "big") for i in range(0, len(b), 2))
    while s > 0xFFFF:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def reference(frames):
    """[(head index, output bytes)] in output order, and the set of input frames that went into an output."""
    frags, outs, used = {}, {}, set()
    for i, f in enumerate(frames):
        if f is None or len(f) > 65535:
            continue
        v4 = len(f) >= 34 and f[12] == 8 and f[13] == 0 and f[14] >> 4 == 4 and (f[14] & 15) >= 5
        if v4:
            ihl, tl = (f[14] & 15) * 4, f[16] * 256 + f[17]
            v4 = 14 + ihl <= len(f) and ihl <= tl and 14 + tl <= len(f)
        if not v4 or (f[20] & 0x3F) == 0 and f[21] == 0:
            outs[i] = bytes(f)
            used.add(i)
            continue
        start = ((f[20] & 0x1F) * 256 + f[21]) * 8
        frags.setdefault((f[18:20], f[23], f[26:34]), []).append((start, i, bool(f[20] & 0x20), f[14 + ihl:14 + tl], ihl))
    for parts in frags.values():
        parts = sorted(parts)
        end, good = 0, True
        for n, (start, i, more, body, ihl) in enumerate(parts):
            last = n == len(parts) - 1
            good &= start == end and more != last and (len(body) >= 1 if last else len(body) >= 8 and len(body) % 8 == 0)
            end = start + len(body)
        if not good or parts[0][4] + end > 65535:
            continue
        first = frames[parts[0][1]]
        buf = bytearray(first[:14 + parts[0][4]]) + bytearray(end)
        for start, i, more, body, ihl in parts:
            buf[14 + parts[0][4] + start:14 + parts[0][4] + start + len(body)] = body
            used.add(i)
        buf[16:18] = (parts[0][4] + end).to_bytes(2, "big")
        buf[20] &= 0xC0
        buf[21] = 0
        buf[24:26] = b"\0\0"
        buf[24:26] = (0xFFFF - ones_sum(bytes(buf[14:14 + parts[0][4]]))).to_bytes(2, "big")
        outs[parts[0][1]] = bytes(buf)
    return sorted(outs.items()), used


def check_against_reference(name, frames):
    out, src, rows, collided = reassemble_host(frames)
    want, used = reference(frames)
    assert [i for i, _ in want] == list(src), name
    assert [b for _, b in want] == out, name
    gone = np.isin(rows["kind"], (abi.REASM_PASS, abi.REASM_HEAD, abi.REASM_PART))
    assert set(np.flatnonzero(gone)) == used, name
    # the rows are consistent with the outputs
    for i, r in enumerate(rows):
        if r["kind"] in (abi.REASM_PASS, abi.REASM_HEAD):
            assert src[r["out"]] == i, (name, i)
        if r["kind"] == abi.REASM_HEAD:
            assert r["head"] == i and r["members"] == int((rows["head"] == i).sum()) >= 2, (name, i)
            assert len(out[r["out"]]) == 14 + int(r["hdr_len"]) + int(r["data_len"]), (name, i)
        elif r["kind"] == abi.REASM_PART:
            assert rows[r["head"]]["kind"] == abi.REASM_HEAD and r["out"] == rows[r["head"]]["out"], (name, i)
        else:
            assert r["head"] == abi.REASM_NO_INDEX and r["members"] == 0 and r["data_len"] == 0, (name, i)
        if r["kind"] in (abi.REASM_HELD, abi.REASM_NONE):
            assert r["out"] == abi.REASM_NO_INDEX, (name, i)
        assert r["status"] == (abi.ERR_BAD_EXTENT if frames[i] is None else abi.FRAME_OK), (name, i)
    return out, src, rows, collided


@pytest.mark.parametrize("case", range(len(rf.cases())), ids=[n for n, _, _ in rf.cases()])
def test_every_case_equals_the_independent_reference(case):
    name, classes, frames = rf.cases()[case]
    out, src, rows, collided = check_against_reference(name, frames)
    held = rows["kind"] == abi.REASM_HELD
    incomplete = {"missing first", "missing middle", "missing last", "duplicate", "overlap", "gap of 8", "last with MF",
                  "middle without MF", "data not a multiple of 8", "zero data", "65536", "input was a fragment"}
    if classes & incomplete:
        assert held.any(), name
    if classes & {"in order", "reversed", "shuffled", "interleaved", "same addresses, other id", "same id, other addresses",
                  "head options, parts none", "trailing bytes"} and "65536" not in classes:
        assert not held.any() and (rows["kind"] == abi.REASM_HEAD).any(), name
    if name == "hl + D is 65535":
        assert len(out) == 1 and len(out[0]) == 14 + 65535
    if name == "hl 60 + D is 65535 / 65536":
        assert [tuple(r) for r in rows[["kind", "data_len"]]] == [(abi.REASM_HEAD, 65475), (abi.REASM_PART, 0),
                                                                   (abi.REASM_HELD, 0), (abi.REASM_HELD, 0)]
    if name == "pass-through":
        assert list(rows["kind"]) == [abi.REASM_PASS, abi.REASM_NONE] + [abi.REASM_PASS] * 6 + [abi.REASM_NONE] + [abi.REASM_PASS] * 3
        assert out == [f for f in frames if f is not None]


def test_the_whole_table_and_the_long_train():
    frames, owner = rf.table()
    check_against_reference("table", frames)
    t = list(rf.long_train())
    random.Random(5).shuffle(t)
    out, src, rows, _ = check_against_reference("8183 pieces", t)
    assert len(out) == 1 and rows[src[0]]["members"] == 8183
    want = rf.retag(dict(ff.corpus())["65535 bytes, hl 60"], 0x7500)
    assert out[0] == want


@pytest.mark.parametrize("mtu", rf.MTUS)
def test_fragment_shuffle_reassemble_is_the_identity(oracle, mtu):
    """reassemble_host(shuffled fragment_host(x)) == x byte for byte for every
    whole datagram with DF clear and len == 14 + TL; the documented difference
    for the others: bytes past 14 + TL are dropped from a datagram that was
    split, a frame fragment_host gave no piece for (DF set, bad extent,
    offset overflow) is absent, and the pieces of an input that was itself a
    fragment stay HELD. Every output parses to the record of its original."""
    names = [n for n, _ in ff.corpus()]
    frames = [None if f is None else rf.retag(f, 0x100 + i) if rf.is_ipv4(f) else f for i, f in enumerate(ff.frames())]
    pieces, psrc, frows = fragment_host(frames, mtu)
    perm = list(range(len(pieces)))
    random.Random(mtu).shuffle(perm)
    out, src, rows, collided = reassemble_host([pieces[p] for p in perm])
    assert not collided.any()
    origin = [int(psrc[perm[s]]) for s in src]  # the input frame of each output
    assert len(set(origin)) == len(origin)
    got = dict(zip(origin, out))
    exact = {i for i, (n, f) in enumerate(zip(names, frames)) if (n, ff.frames()[i]) in set(rf.sources())}
    assert len(exact) > 100
    for i, f in enumerate(frames):
        kind = frows["kind"][i]
        if i in exact:
            assert got[i] == f, names[i]
        elif kind == abi.FRAG_PASS:
            # a pass-through that is itself a fragment is HELD on the way back; anything else comes back as it is
            if classify_frame(f)[1] == abi.REASM_HELD:
                assert i not in got, names[i]
            else:
                assert got[i] == f, names[i]
        elif kind == abi.FRAG_SPLIT:
            word = int.from_bytes(f[20:22], "big")
            if word & 0x3FFF:
                assert i not in got, names[i]  # the input was a fragment: never complete
            else:
                assert got[i] == ff.datagram(f), names[i]  # the bytes past 14 + TL are gone
        else:
            assert i not in got, names[i]
        if i in got and len(got[i]) >= 34 and len(got[i]) <= 65535:
            a, b = oracle.parse_frame(got[i]), oracle.parse_frame(f[:len(got[i])] if kind == abi.FRAG_SPLIT else f)
            assert a.tobytes() == b.tobytes(), names[i]


def test_truth_table_of_the_completeness_rules():
    M = lambda *m: [(20, fo, mf, d) for fo, mf, d in m]  # noqa: E731
    assert datagram_complete(M((0, 1, 8), (1, 0, 1)))
    assert datagram_complete(M((0, 1, 16), (2, 1, 8), (3, 0, 5)))
    assert not datagram_complete(M((1, 1, 8), (2, 0, 1)))              # member 0 not at 0
    assert not datagram_complete(M((0, 1, 8), (2, 0, 1)))              # a gap
    assert not datagram_complete(M((0, 1, 16), (1, 0, 9)))             # an overlap
    assert not datagram_complete(M((0, 1, 8), (0, 1, 8), (1, 0, 1)))   # a duplicate
    assert not datagram_complete(M((0, 1, 4), (1, 0, 1)))              # d below 8 in front of another
    assert not datagram_complete(M((0, 1, 12), (1, 0, 1)))             # d not a multiple of 8: the next does not start there
    assert not datagram_complete(M((0, 1, 0), (0, 0, 9)))              # no data in front of another
    assert not datagram_complete(M((0, 0, 8), (1, 0, 1)))              # MF clear in the middle
    assert not datagram_complete(M((0, 1, 8), (1, 1, 1)))              # MF set on the last
    assert not datagram_complete(M((0, 1, 8), (1, 0, 0)))              # the last without data
    assert not datagram_complete(M((0, 1, 8)))                         # a lone first
    assert not datagram_complete(M((3, 0, 8)))                         # a lone last
    assert datagram_complete([(20, 0, 1, 32760), (20, 4095, 0, 32755)])      # 20 + 65515 = 65535
    assert not datagram_complete([(20, 0, 1, 32760), (20, 4095, 0, 32756)])
    assert datagram_complete([(60, 0, 1, 32760), (20, 4095, 0, 32715)])      # the head's hl counts
    assert not datagram_complete([(60, 0, 1, 32760), (20, 4095, 0, 32716)])
    assert datagram_complete([(20, 0, 1, 32760), (60, 4095, 0, 32755)])      # a part's does not


def test_the_pinned_collision():
    a, b = rf.SRC_A + rf.DST_C + bytes([0, 17, 0, 0]), rf.SRC_B + rf.DST_C + bytes([0, 17, 0, 0])
    assert a != b and toeplitz(a) == toeplitz(b)
    assert key_hash((rf.SRC_A, rf.DST_C, 17, 1)) == key_hash((rf.SRC_B, rf.DST_C, 17, 2)) == toeplitz(a)
    name, _, frames = next(c for c in rf.cases() if c[0] == "collision")
    out, src, rows, collided = reassemble_host(frames)            # exact: all three datagrams come out
    assert list(collided) == [True, True, False, True, True, True, False, True]
    assert len(out) == 3 and (rows["flags"] == 0).all() and not (rows["kind"] == abi.REASM_HELD).any()
    out_d, src_d, rows_d, collided_d = reassemble_host(frames, exact=False)  # as the device: the mixed run is held
    assert (collided_d == collided).all() and len(out_d) == 1 and list(src_d) == [6]
    assert (rows_d["kind"][collided] == abi.REASM_HELD).all() and (rows_d["flags"][collided] == abi.REASM_COLLISION).all()
    assert (rows_d["flags"][~collided] == 0).all()
    # the rows differ at the collided frames only
    same = rows_d[~collided].copy()
    same["out"] = rows[~collided]["out"]  # the output numbering moves with the outputs in front
    assert (same == rows[~collided]).all()


def test_pack_host_and_a_bad_align():
    out = [b"abc", b"", b"defgh"]
    data, offs = pack_host(out, 4)
    assert list(offs) == [0, 4, 4, 12] and data == b"abc\0defgh\0\0\0"
    assert pack_host(out, 1)[0] == b"abcdefgh"
    with pytest.raises(ValueError):
        reassemble_host([], align=3)
