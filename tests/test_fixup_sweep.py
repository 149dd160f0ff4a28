"""CPU: the fix-up / checksum sweep of tests/fixup_sweep.py before it runs on
the device: the corpus holds what the sweep relies on, the two references
agree on all of it, the kernels' per-frame cores (checksum_core.hpp, run on
the host through tests/native/core_harness.hip behind the kernels' own
frame_extent) equal the oracle in every table layout and at every 16-B phase,
whole buffer included, and the comparer catches each seeded defect and names
its place. tests/test_gpu_fixup_sweep.py repeats the comparison on the GPU;
tests/test_core_harness.py runs the same cores under the sanitizers."""
import numpy as np
import pytest

from nex_amd import abi
from tests import fixup_sweep as fs
from tests.native import harness

MODE_IDS = [f"{'from_ip' if m[0] else 'eth'}{m[1]}" for m in fs.MODES]
LO = fs.GUARD_BEFORE


def test_corpus_conditions(oracle):
    rep = fs.check_corpus()
    assert len(rep) == len(fs.corpus().frames)


@pytest.mark.parametrize("mode", fs.MODES, ids=MODE_IDS)
def test_fixup_ref_equals_oracle(oracle, mode):
    frames = fs.mode_frames(*mode)
    for which in fs.WHICH:
        fixed, rep = fs.oracle_fixed(frames, which, *mode)
        for i, f in enumerate(frames):
            got, row = fs.fixup_ref(f, which, *mode)
            assert got == fixed[i], (which, i, f[:96].hex())
            assert row == fs.report_row(rep[i]), (which, i, row, rep[i])


def test_checksum_references(oracle):
    """oracle.checksum == RFC 1071 with the skipped word zeroed, the dropped
    trailing byte of an odd buffer included; the out-of-range entries are 0 by
    the kernel's extent rule (an empty buffer by the reference's too)."""
    dropped = 0
    for b in fs.checksum_cases():
        if b.want is None:
            assert oracle.checksum(b.data, b.skipword) == fs.checksum_ref(b.data, b.skipword), (len(b.data), b.skipword)
            dropped += len(b.data) % 2 == 1 and 2 * b.skipword == len(b.data) - 1 and b.data[-1] != 0
        else:
            assert b.want == 0 and (len(b.data) == 0 or len(b.data) > fs.MAX_FRAME)
    assert oracle.checksum(b"", 0) == 0
    assert dropped >= 20
    odd = b"\x12\x34\x56"
    assert oracle.checksum(odd, 1) == fs.rfc1071(b"\x12\x34") != oracle.checksum(odd, 2)


# ---------------------------------------------------------------- harness parity

def guarded(data):
    """`data` inside GUARD_FILL guards, at the same 16-B phase; (whole buffer, the data view)."""
    buf = fs.aligned(LO + len(data) + fs.GUARD_AFTER, fs.GUARD_FILL)
    buf[LO:LO + len(data)] = data
    return buf, buf[LO:LO + len(data)]


def check_recompute(lay, fixed, rep, which, mode, report=True):
    keep = range(len(fixed)) if lay.keep is None else lay.keep
    want = fs.expected_buffer(lay.data, lay.offsets, lay.lengths, [fixed[i] for i in keep])
    buf, data = guarded(lay.data)
    got = harness.recompute(data, flags=fs.parse_flags(mode[0]), ip_offset=mode[1], which=which, report=report,
                            **lay.table)
    fs.compare(buf, want, lay.offsets, lay.lengths, got, rep[np.asarray(keep)] if report else None, lo=LO,
               what=f"{lay.name} which {which} mode {mode}")
    return buf


@pytest.mark.parametrize("which", fs.WHICH)
@pytest.mark.parametrize("mode", fs.MODES, ids=MODE_IDS)
def test_harness_recompute_matches_oracle(oracle, which, mode):
    frames = fs.mode_frames(*mode)
    fixed, rep = fs.oracle_fixed(frames, which, *mode)
    names = []
    for lay in fs.host_layouts(frames, shift=1):
        check_recompute(lay, fixed, rep, which, mode)
        names.append(lay.name)
    assert names == ["packed u64", "packed u32", "packed u32 + bases", "offsets + lengths u64", "offsets32 + lengths",
                     "strided + lengths", "strided"]
    check_recompute(fs.host_layouts(frames, shift=1)[0], fixed, rep, which, mode, report=False)


def test_harness_recompute_every_phase(oracle):
    """The first frame at every phase 0..15 mod 16 (the shift in the offsets,
    the base aligned), every layout; both address parities and every phase of
    the L4 range's start occur among the frames fixed at L4."""
    frames = fs.corpus().frames
    fixed, rep = fs.oracle_fixed(frames, fs.BOTH, False, 0)
    seen = set()
    for shift in range(16):
        for lay in fs.host_layouts(frames, shift=shift):
            check_recompute(lay, fixed, rep, fs.BOTH, (False, 0))
            if lay.name == "packed u64":
                l4 = (rep["done"] & abi.FIX_L4) != 0
                seen |= set(((lay.offsets[l4] + rep["l4_off"][l4]) % 16).tolist())
    assert seen == set(range(16))


def grouped_checksum_cases():
    groups = {}
    for b in fs.checksum_cases():
        groups.setdefault(b.skipword, []).append(b)
    return groups


def test_harness_checksum_matches_oracle(oracle):
    for skip, bufs in grouped_checksum_cases().items():
        want = np.array([oracle.checksum(b.data, skip) if b.want is None else b.want for b in bufs], np.uint16)
        datas = [b.data for b in bufs]
        for shift in (0, 1, 2, 3, 15):
            for lay in fs.host_layouts(datas, shift=shift):
                got = harness.checksum(lay.data, skipword=skip, **lay.table)
                w = want if lay.keep is None else want[lay.keep]
                assert (got == w).all(), (skip, shift, lay.name, np.nonzero(got != w)[0][:5], got[got != w][:5])


def test_harness_refuses_bad_extents(oracle):
    """frame_extent's refusals on the host: the row is zero and no byte changes."""
    f = fs.corpus().frames[0]
    data, _ = fs.pack([f], shift=0, tail=0)
    n = len(data)
    offs = np.array([0, 0, n, n, n + 1, n - 4, 0], np.int64)
    lens = np.array([65536, 70000, 0, 1, 0, 5, len(f)], np.int64)
    buf, d = guarded(data)
    rep = harness.recompute(d, offsets=offs, lengths=lens)
    want = fs.expected_buffer(data, offs[-1:], lens[-1:], [fs.oracle_fixed((f,), fs.BOTH, False, 0)[0][0]])
    fs.compare(buf, want, offs, lens, lo=LO, what="bad extents")
    assert not rep[:6].view(np.uint64).any() and rep[6]["done"] == fs.BOTH
    assert list(harness.checksum(data, offsets=offs, lengths=lens, skipword=5)[:6]) == [0] * 6


# ---------------------------------------------------------------- seeded defects

@pytest.fixture(scope="module")
def correct(oracle):
    """A correct result over the structured frames under 600 B, packed from
    byte 1 between guards: (frames, buffer, expected data, offsets, lengths,
    report, unfixed data)."""
    c = fs.corpus()
    frames = [c.frames[i] for i in c.structured if len(c.frames[i]) < 600]
    fixed, rep = fs.oracle_fixed(tuple(frames), fs.BOTH, False, 0)
    lay = fs.host_layouts(frames, shift=1)[0]
    buf = check_recompute(lay, fixed, rep, fs.BOTH, (False, 0))
    want = fs.expected_buffer(lay.data, lay.offsets, lay.lengths, fixed)
    for a in (buf, want, lay.data):
        a.setflags(write=False)
    return frames, buf, want, lay.offsets, lay.lengths, rep, lay.data


def pick(correct, cond):
    """The first frame fixed at L4 that satisfies cond(i, field position in the buffer)."""
    frames, buf, want, offs, lens, rep, _ = correct
    for i in range(len(frames)):
        if rep[i]["done"] & abi.FIX_L4:
            sk = {17: 6, 6: 16, 1: 2, 58: 2}[int(rep[i]["proto"])]
            at = LO + int(offs[i]) + int(rep[i]["l4_off"]) + sk
            if cond(i, at):
                return i, at
    raise AssertionError("the corpus holds no such frame")


def expect(correct, buf, rep, i, off):
    _, _, want, offs, lens, wrep, _ = correct
    with pytest.raises(AssertionError, match=rf"frame {i} \(lane {i % 256}\) offset {off} of {int(lens[i])},"):
        fs.compare(buf, want, offs, lens, rep, wrep, lo=LO, what="seeded")


def put(buf, at, value):
    buf[at], buf[at + 1] = value >> 8, value & 0xFF


def test_compare_accepts_the_correct_result(correct):
    _, buf, want, offs, lens, rep, _ = correct
    fs.compare(buf, want, offs, lens, rep.copy(), rep, lo=LO)


def test_seeded_swapped_multiplier(correct):
    """wsum's multiplier of an odd-start range swapped: the value rotated by 8."""
    i, at = pick(correct, lambda i, at: (at - LO) % 2 == 1 and correct[1][at] != correct[1][at + 1])  # an odd L4 start
    buf, rep = correct[1].copy(), correct[5].copy()
    c = int(rep[i]["l4_csum"])
    rol = ((c << 8) | (c >> 8)) & 0xFFFF
    put(buf, at, rol)
    rep[i]["l4_csum"] = rol
    expect(correct, buf, rep, i, at - LO - int(correct[3][i]))


def test_seeded_dropped_carry(correct):
    """One end-around carry dropped: the sum one short, the checksum one over."""
    i, at = pick(correct, lambda i, at: True)
    buf, rep = correct[1].copy(), correct[5].copy()
    c = (int(rep[i]["l4_csum"]) + 1) & 0xFFFF
    put(buf, at, c)
    rep[i]["l4_csum"] = c
    first = at if (c >> 8) != correct[1][at] else at + 1
    expect(correct, buf, rep, i, first - LO - int(correct[3][i]))


def test_seeded_last_odd_byte_left_out(correct):
    frames = correct[0]
    i, at = pick(correct, lambda i, at: (len(frames[i]) - int(correct[5][i]["l4_off"])) % 2 == 1 and frames[i][-1] != 0
                 and frames[i][12:14] == b"\x86\xdd")
    cut, row = fs.fixup_ref(frames[i][:-1] + b"\0", fs.BOTH)  # the sum without the last byte
    buf, rep = correct[1].copy(), correct[5].copy()
    assert row[3] != int(rep[i]["l4_csum"])
    put(buf, at, row[3])
    rep[i]["l4_csum"] = row[3]
    first = at if (row[3] >> 8) != correct[1][at] else at + 1
    expect(correct, buf, rep, i, first - LO - int(correct[3][i]))


def test_seeded_field_one_byte_early(correct):
    unfixed = correct[6]
    i, at = pick(correct, lambda i, at: correct[1][at - 1] != correct[1][at])
    buf = correct[1].copy()
    c = int(correct[5][i]["l4_csum"])
    put(buf, at - 1, c)
    buf[at + 1] = unfixed[at + 1 - LO]
    expect(correct, buf, correct[5], i, at - 1 - LO - int(correct[3][i]))


def test_seeded_neighbour_clobbered(correct):
    i, at = pick(correct, lambda i, at: i + 1 < len(correct[0]))
    buf = correct[1].copy()
    buf[LO + int(correct[3][i + 1])] ^= 0x40
    expect(correct, buf, correct[5], i + 1, 0)


def test_seeded_done_but_unwritten(correct):
    unfixed = correct[6]
    i, at = pick(correct, lambda i, at: unfixed[at - LO] != correct[1][at])
    buf = correct[1].copy()
    buf[at:at + 2] = unfixed[at - LO:at - LO + 2]
    expect(correct, buf, correct[5], i, at - LO - int(correct[3][i]))


def test_seeded_byte_after_data(correct):
    _, buf, want, offs, lens, rep, _ = correct
    b = buf.copy()
    b[LO + len(want)] = 0
    with pytest.raises(AssertionError, match="byte written after data: 0 B past its end"):
        fs.compare(b, want, offs, lens, rep, rep, lo=LO)
    b = buf.copy()
    b[LO - 1] = 0
    with pytest.raises(AssertionError, match="byte written before data: 1 B ahead"):
        fs.compare(b, want, offs, lens, rep, rep, lo=LO)


def test_seeded_gap_and_report(correct, oracle):
    """A pad byte between two frames, and a report row that differs in one field."""
    frames = correct[0][:40]
    fixed, rep = fs.oracle_fixed(tuple(frames), fs.BOTH, False, 0)
    lay = next(l for l in fs.host_layouts(frames, shift=0) if l.name == "offsets + lengths u64")
    i = next(i for i, f in enumerate(frames) if len(f) % 4 and i + 1 < len(frames))
    buf = check_recompute(lay, fixed, rep, fs.BOTH, (False, 0))
    want = fs.expected_buffer(lay.data, lay.offsets, lay.lengths, fixed)
    gap = buf.copy()
    gap[LO + int(lay.offsets[i] + lay.lengths[i])] = 0x77
    with pytest.raises(AssertionError, match=rf"in the gap after frame {i} \(lane {i}\), 0 B past its end"):
        fs.compare(gap, want, lay.offsets, lay.lengths, rep, rep, lo=LO)
    bad = rep.copy()
    bad[7]["l4_off"] += 1
    with pytest.raises(AssertionError, match=r"first frame 7 \(lane 7\): \(got, want\) \{'l4_off'"):
        fs.compare(buf, want, lay.offsets, lay.lengths, bad, rep, lo=LO)
