"""GPU: the geometry sweep of tests/span_geometry.py through the parse kernels,
bit for bit against the oracle on the same layout, in every output kind, with
64 guard bytes on both sides of every output.

k_parse_span: a probe at every byte position of its head window around a
sub-tile edge (16-KiB edges for records, 24-KiB ones for the other kinds; a
batch aimed at one size is one more valid batch for the other), frame ends,
IP ends and group ends at every phase of an edge, prefix sums that wrap 2^32,
the bucketed generic pass and its deferred-range loop; packed at four
first-frame shifts on u64 and u32 tables, offsets + lengths with the monotone
hint and 16-B gaps, a fixed stride of 200; lenient everywhere, strict, from-IP
and VLAN on the unshifted batch. k_tail_sums / k_parse_lane80 (offsets +
lengths without the hint): tail ranges against piece and chunk edges, piece
totals that leave quarter-waves idle, the window at the end of the data, one
wave spanning more than 2^31 bytes. tests/test_span_geometry.py asserts on the
CPU that every class is covered and every probe sits where its case says.

Sizes: the unshifted batch of classes 1-3 holds 4679 cases (37 probes x 117
head positions, the end and span-end sweeps) in 36097 frames, 77 MB aimed at
16384 and 115 MB at 24576; the four shifted / gapped layouts carry the ten
CORE_PROBES (1520 cases, 25 / 37 MB); 145 small batches per sub-tile size end
the data at hi. Wall time on an MI355X: the file 4.8 s, 1.4 s of it the engine
and oracle fixtures; the slowest test (the unshifted 16384 batch in four parse
modes, which also builds the probes) 1.3 s, every other one under 0.4 s.

No case disagreed with the oracle when this suite was written."""
import numpy as np
import pytest

from nex_amd import abi
from nex_amd.frame import ParseMode, ParseOption
from tests import span_geometry as sg

pytestmark = pytest.mark.gpu

SUBS = sorted(set(sg.SPAN_SUB.values()))
MODES = [(ParseOption(), ParseMode.Strict), (ParseOption(True, 14), ParseMode.Lenient),
         (ParseOption(unwrap_vlan=True), ParseMode.Lenient)]


def lengths_of(lay):
    return np.array([len(f) for f in lay.frames], np.int64)


def sweep(engine, oracle, lay, what, modes=()):
    """One layout in every output kind, on the u64 and the u32 table."""
    data, offs, lens = lay.table()
    hints = 0 if lens is None else abi.FRAMES_MONOTONE
    batch = sg.device_batch(data, offs, lens, hints)
    n = lengths_of(lay)
    want = oracle.parse_packed(data, offs, lens)
    sg.check(engine, batch, want, n, lay.cases, what)
    sg.check(engine, batch.with_offsets32(), want, n, lay.cases, what + " offsets32")
    for opt, mode in modes:
        w = oracle.parse_packed(data, offs, lens, flags=opt.flags(mode), ip_offset=opt.offset)
        sg.check(engine, batch, w, n, lay.cases, f"{what} flags {opt.flags(mode)}", option=opt, mode=mode)


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("shift,gap", [(s, 0) for s in sg.SHIFTS] + [(0, 16)])
def test_sub_tile_edges(engine, oracle, sub, shift, gap):
    """Classes 1-3: head sweep, end sweep and span ends at every edge position."""
    lay = sg.class123(sub, shift, gap)
    sweep(engine, oracle, lay, f"SUB {sub} shift {shift} gap {gap}", MODES if shift == 0 and gap == 0 else ())


@pytest.mark.parametrize("sub", SUBS)
def test_span_ends_at_the_end_of_the_data(engine, oracle, sub):
    """The group's last byte at every phase of an edge with nothing behind it:
    the data tensor ends at hi; last groups of 1, 2, 63, 64, 65, 255 and 256
    frames."""
    for lay in sg.span_end_batches(sub):
        c = lay.cases[-1]
        sweep(engine, oracle, lay, f"data ends at hi, {lay.n} frames, {sg.case_name(c)}")


@pytest.mark.parametrize("shift", [0, 1])
def test_prefix_sums_wrap(engine, oracle, shift):
    sweep(engine, oracle, sg.prefix_wrap(shift), f"prefix wrap shift {shift}")


def test_generic_section(engine, oracle):
    """The declined sets (one lane, 4, 5, a whole wave, all 256 in one and in
    nine buckets) as the groups of one batch, at two shifts."""
    frames = [f for _, fr, _ in sg.generic_groups() for f in fr]
    for shift in (0, 13):
        lay = sg.packed(frames, shift)
        lay.cases = [sg.Case(5, 0, None, None, name, sg.TILE * g, "group")
                     for g, (name, _, _) in enumerate(sg.generic_groups())]
        sweep(engine, oracle, lay, f"generic section shift {shift}", MODES[:1])


def test_deferred_ranges(engine, oracle):
    """Worker waves with 1, 3, 4, 5, 8 and 64 deferred ranges of every length
    and start phase (NEXG_PARSE_VLAN: padded frames' L4 ranges are deferred)."""
    groups = sg.deferred_groups()
    lay = sg.packed([f for _, fr, _ in groups for f in fr])
    lay.cases = [sg.Case(5, 0, None, None, name, sg.TILE * g, "group") for g, (name, _, _) in enumerate(groups)]
    sweep(engine, oracle, lay, "deferred ranges", MODES[2:])


def test_stride_200(engine, oracle):
    arr = sg.stride200()
    batch = sg.device_batch(arr.reshape(-1), None, stride=200, count=len(arr))
    want = oracle.parse_packed(arr.reshape(-1), stride=200)
    sg.check(engine, batch, want, np.full(len(arr), 200, np.int64), (), "stride 200")


def test_two_pass_tail_ranges(engine, oracle):
    data, offs, lens, notes = sg.two_pass_batch()
    batch = sg.device_batch(data, offs, lens)
    cases = [sg.Case(7, 0, None, None, what, 64 * w, "wave") for w, what in notes]
    want = oracle.parse_packed(data, offs, lens)
    sg.check(engine, batch, want, lens.astype(np.int64), cases, "two-pass")
    sg.check(engine, batch.with_offsets32(), want, lens.astype(np.int64), cases, "two-pass offsets32")
    opt, mode = MODES[0]
    sg.check(engine, batch, oracle.parse_packed(data, offs, lens, flags=opt.flags(mode)), lens.astype(np.int64), cases,
             "two-pass strict", option=opt, mode=mode)


def test_two_pass_window_at_the_end_of_the_data(engine, oracle):
    """A 60-B frame at every start phase with the data ending at its end."""
    for data, offs, lens in sg.window_end_batches():
        batch = sg.device_batch(data, offs, lens)
        assert batch.data.numel() == int(offs[-1] + lens[-1])
        want = oracle.parse_packed(data, offs, lens)
        sg.check(engine, batch, want, lens.astype(np.int64), (), f"window end phase {int(offs[-1]) % 16}")


def test_two_pass_wave_over_2_gib(engine, oracle):
    """One wave whose two frames lie more than 2^31 bytes apart in one
    allocation (k_tail_sums' per-lane fallback); only the two ends are written."""
    import torch
    from nex_amd.engine import FrameBatch
    size = (1 << 31) + 8192
    try:
        dev = torch.zeros(size, dtype=torch.uint8, device="cuda")
    except RuntimeError as e:  # torch.OutOfMemoryError is one
        pytest.skip(f"a {size}-B device allocation was refused: {e}")
    frames = [sg.udp4_frame(700, 1), sg.udp4_frame(1200, 2)]
    offs = np.array([259, (1 << 31) + 1030], np.uint64)
    lens = np.array([700, 1200], np.uint32)
    for o, f in zip(offs, frames):
        dev[int(o): int(o) + len(f)] = torch.frombuffer(bytearray(f), dtype=torch.uint8).cuda()
    batch = FrameBatch(data=dev, count=2, offsets=torch.from_numpy(offs.astype(np.int64)).cuda(),
                       lengths=torch.from_numpy(lens.astype(np.int32)).cuda())
    want = oracle.parse_frames(frames)
    ok = abi.C_L4_OK | abi.C_IP_OK
    assert ((want["flags"] & ok) == ok).all()
    sg.check(engine, batch, want, lens.astype(np.int64), (), "two frames over 2 GiB apart")
