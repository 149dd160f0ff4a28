"""GPU: nexg_rewrite_batch (k_rewrite, nex_amd/csrc/nexg_rewrite.hip) through
Engine.rewrite against tests/rewrite_frames.py: the corpus under every action
in both checksum modes on every table layout with the batch base at four byte
phases (the whole data buffer compared, so a store outside a field shows),
the tile-edge counts with every index value, raw IP packets, the
parse -> select -> rewrite composition, 16 384 IMIX frames, the 65535-B frame
and run-to-run identity."""
import numpy as np
import pytest

from nex_amd import abi
from nex_amd.engine import FrameBatch
from nex_amd.frame import ParseOption
from nex_amd.rewrite import rewrite_host
from nex_amd.select import Filter, Rule
from tests import helpers
from tests import rewrite_frames as rf

pytestmark = pytest.mark.gpu

GAP = 0xA5
PHASES = (0, 1, 7, 15)


# ---- layouts over host arrays: (data, offsets, lengths, batch) ----------------------------

def _place(frames, offs, total):
    buf = np.full(total, GAP, np.uint8)
    for f, o in zip(frames, offs):
        buf[o:o + len(f)] = np.frombuffer(f, np.uint8)
    return buf


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def layout(name, frames, phase):
    """The frames in layout `name`, the first one `phase` bytes into a 16-B
    block (device allocations are 256-B aligned), every byte outside a frame
    0xA5. The fixed-stride layout takes the most common length only."""
    lens = np.array([len(f) for f in frames], np.int64)
    keep = np.arange(len(frames))
    if name == "stride":
        width = int(np.bincount(lens).argmax())
        keep = np.nonzero(lens == width)[0]
        frames = [frames[i] for i in keep]
        stride = width + phase  # data stays 4-B aligned: the phase walks through the frames instead
        offs = np.arange(len(frames), dtype=np.int64) * stride
        data = _place(frames, offs, len(frames) * stride + 16)
        return data, offs, lens[keep], keep, FrameBatch(data=_dev(data), count=len(frames), stride=stride,
                                                        lengths=_dev(lens[keep].astype(np.int32)))
    gaps = np.array([i % 7 for i in range(len(frames))], np.int64) if name == "offsets + lengths" else np.zeros(len(frames), np.int64)
    offs = np.zeros(len(frames) + 1, np.int64)
    offs[1:] = np.cumsum(lens + gaps)
    offs += phase
    data = _place(frames, offs[:-1], int(offs[-1]) + 16)
    if name == "offsets + lengths":
        b = FrameBatch(data=_dev(data), count=len(frames), offsets=_dev(offs[:-1]), lengths=_dev(lens.astype(np.int32)))
    else:
        b = FrameBatch(data=_dev(data), count=len(frames), offsets=_dev(offs))
        if name == "packed u32":
            b = b.with_offsets32()
    return data, offs[:-1], lens, keep, b


LAYOUTS = ("packed", "offsets + lengths", "packed u32", "stride")


def expected(data, offs, frames_out):
    want = data.copy()
    for f, o in zip(frames_out, offs):
        want[o:o + len(f)] = np.frombuffer(f, np.uint8)
    return want


def check(engine, batch, data, offs, want_frames, want_rows, actions, index, what, option=ParseOption()):
    idx = None if index is None else _dev(np.asarray(index, np.uint8))
    rows = engine.rewrite(batch, actions, idx, option)
    got = batch.data.cpu().numpy()
    want = expected(data, offs, want_frames)
    bad = np.nonzero(got != want)[0]
    if len(bad):
        p = int(bad[0])
        i = int(np.searchsorted(offs, p, side="right")) - 1
        raise AssertionError(f"{what}: {len(bad)} bytes differ; first at data byte {p} (frame {i}, lane {i % 256}, "
                             f"offset {p - int(offs[i])} of {len(want_frames[i])}): got {got[p]:#04x}, want {want[p]:#04x}")
    r = helpers.to_host(rows, abi.REWRITTEN_DTYPE, batch.count)
    bad = np.nonzero(r != want_rows)[0]
    assert len(bad) == 0, (what, len(bad), int(bad[0]), r[bad[0]], want_rows[bad[0]])


# ---- the corpus ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def corpus(oracle):
    return rf.corpus()


@pytest.mark.parametrize("name", LAYOUTS)
@pytest.mark.parametrize("incremental", (False, True), ids=("recompute", "incremental"))
def test_corpus_every_action_layout_and_phase(engine, corpus, incremental, name):
    halves = (corpus.fixed, corpus.garbage)
    for first, acts in rf.action_chunks():
        frames, index, want_frames, want_rows = [], [], [], []
        for half in halves:
            ref = rf.ref_all(half, incremental)
            keep = rf.small(half)
            for j in range(len(acts)):
                out, rows = ref[first + j]
                frames += [half[i] for i in keep]
                index += [j] * len(keep)
                want_frames += [out[i] for i in keep]
                want_rows.append(rows[keep])
        want_rows = np.concatenate(want_rows)
        for phase in PHASES:
            data, offs, lens, keep, batch = layout(name, frames, phase)
            assert batch.count >= (100 if name == "stride" else 5000)
            check(engine, batch, data, offs, [want_frames[i] for i in keep], want_rows[keep], rf.to_set(acts, incremental),
                  [index[i] for i in keep], f"{name} phase {phase} actions {first}..")


@pytest.mark.parametrize("incremental", (False, True), ids=("recompute", "incremental"))
def test_counts_and_every_index_value(engine, corpus, incremental):
    _, acts = rf.action_chunks()[0]
    assert len(acts) == 16
    actions = rf.to_set(acts, incremental)
    pool = [corpus.garbage[i] for i in rf.small(corpus.garbage)]
    values = list(range(16)) + [abi.ACTION_NONE, 16, 77]
    for count in (0, 1, 255, 256, 257, 513):
        frames = [pool[(3 * i) % len(pool)] for i in range(count)]
        index = [values[i % len(values)] for i in range(count)]
        for idx in (index, None):
            want_frames, want_rows = rewrite_host(frames, actions, idx)
            data, offs, lens, keep, batch = layout("packed", frames, 1)
            check(engine, batch, data, offs, want_frames, want_rows, actions, idx, f"count {count} index {idx is not None}")
    # one action only: every index but 0 is past the set
    one = rf.to_set(acts[11:12], incremental)
    frames = [pool[i % len(pool)] for i in range(300)]
    index = [values[i % len(values)] for i in range(300)]
    want_frames, want_rows = rewrite_host(frames, one, index)
    assert int((want_rows["action"] == 0).sum()) == 300 // len(values) + 1
    assert int((want_rows["action"] == abi.ACTION_NONE).sum()) == 300 - (300 // len(values) + 1)
    data, offs, lens, keep, batch = layout("packed", frames, 0)
    check(engine, batch, data, offs, want_frames, want_rows, one, index, "one action")


@pytest.mark.parametrize("k", rf.RAW_OFFSETS)
def test_raw_ip_packets(engine, corpus, k):
    opt = ParseOption(from_ip_packet=True, offset=k)
    first, acts = rf.action_chunks()[0]
    for incremental in (False, True):
        for half in rf.raw_ip(k):
            ref = rf.ref_all(half, incremental, abi.PARSE_FROM_IP, k)
            frames = list(half) * len(acts)
            index = [j for j in range(len(acts)) for _ in half]
            want_frames = [f for j in range(len(acts)) for f in ref[first + j][0]]
            want_rows = np.concatenate([ref[first + j][1] for j in range(len(acts))])
            data, offs, lens, keep, batch = layout("packed", frames, 7)
            check(engine, batch, data, offs, want_frames, want_rows, rf.to_set(acts, incremental), index,
                  f"raw ip offset {k} incremental {incremental}", opt)


# ---- composition -----------------------------------------------------------------------------

@pytest.mark.parametrize("incremental", (False, True), ids=("recompute", "incremental"))
def test_select_then_rewrite_is_a_match_action_table(engine, oracle, corpus, incremental):
    from nex_amd.rewrite import Action, ActionSet
    frames = [corpus.fixed[i] for i in rf.small(corpus.fixed)]
    flt = Filter([Rule.udp(), Rule.tcp(), Rule.proto(1)])
    actions = ActionSet([Action.nat4(src="192.0.2.1", dst="198.51.100.7") & Action.ports(40000, 443) & Action.dec_ttl(1),
                         Action.nat6(src="2001:db8::1", dst="2001:db8::2") & Action.ports(dst=8443),
                         Action.set_ttl(7) & Action.mac(dst="02:00:00:00:00:01")], incremental=incremental)
    data, offs, lens, keep, batch = layout("packed", frames, 1)
    rec = engine.parse(batch, out_kind=abi.OUT_RECORD)
    before = helpers.to_host(rec, abi.RECORD_DTYPE, len(frames))
    idx, sel, rule = engine.select(batch, rec, flt, want_rule=True)
    rows = engine.rewrite(sel, actions, rule)
    idx, rule = idx.cpu().numpy().view(np.uint32), rule.cpu().numpy()
    assert all(int((rule == j).sum()) >= 10 for j in range(3)) and len(idx) < len(frames)
    want_sel, want_rows = rewrite_host([frames[i] for i in idx], actions, rule)
    want = list(frames)
    for i, f in zip(idx, want_sel):
        want[i] = f
    got = batch.data.cpu().numpy()
    assert (got == expected(data, offs, want)).all()  # unselected frames and the gaps included
    assert (helpers.to_host(rows, abi.REWRITTEN_DTYPE, len(idx)) == want_rows).all()
    after = helpers.to_host(engine.parse(batch, out_kind=abi.OUT_RECORD), abi.RECORD_DTYPE, len(frames))
    helpers.records_equal(after, oracle.parse_frames(want), want, "records after the rewrite")
    ok = abi.C_IP_OK | abi.C_L4_OK
    for bit in (abi.C_IP_OK, abi.C_L4_OK):
        had = before["flags"] & bit != 0
        if incremental:  # a later fragment's "L4 checksum" covers rewritten addresses it is not updated for
            had &= ~((before["flags"] & abi.L_IPV4 != 0) & (before["ip_word"] & 0x1FFF != 0)) | (bit == abi.C_IP_OK)
        assert (after["flags"][had] & bit != 0).all()
    assert int((before["flags"] & ok == ok).sum()) >= 50
    udp4 = [i for i, r in zip(idx, rule) if r == 0 and before["flags"][i] & abi.L_UDP and before["flags"][i] & abi.L_IPV4
            and (incremental is False or before["ip_word"][i] & 0x1FFF == 0)]
    assert len(udp4) >= 20
    for i in udp4:
        a, b = after[i], before[i]
        assert (int(a["ip_src"]), int(a["ip_dst"])) == (0xC0000201, 0xC6336407)
        assert (int(a["src_port"]), int(a["dst_port"])) == (40000, 443)
        assert int(a["ip_ttl"]) == max(int(b["ip_ttl"]) - 1, 0)
    tcp6 = [i for i, r in zip(idx, rule) if r == 1 and before["flags"][i] & abi.L_TCP and before["flags"][i] & abi.L_IPV6]
    assert len(tcp6) >= 10 and all(int(after["dst_port"][i]) == 8443 and int(after["src_port"][i]) == int(before["src_port"][i])
                                   for i in tcp6)
    icmp = [i for i, r in zip(idx, rule) if r == 2 and before["flags"][i] & abi.L_IPV4]
    assert len(icmp) >= 10 and all(int(after["ip_ttl"][i]) == 7 for i in icmp)


# ---- bulk, ceiling, identity ----------------------------------------------------------------------

def imix_frames(engine, count):
    b = engine.gen_batch(abi.WL_IMIX, count)
    data = b.data.cpu().numpy()
    offs = b.offsets.cpu().numpy().astype(np.int64)
    return b, data, offs, [data[offs[i]:offs[i + 1]].tobytes() for i in range(count)]


@pytest.mark.parametrize("incremental", (False, True), ids=("recompute", "incremental"))
def test_imix_16384_nat_dec_ttl(engine, oracle, incremental):
    batch, data, offs, frames = imix_frames(engine, 16384)
    got = [rf.rewrite_ref(f, rf.NAT44, 0, incremental) for f in frames]
    want_rows = np.array([r for _, r in got], abi.REWRITTEN_DTYPE)
    # IPv4 frames take the whole action, IPv6 frames the ports and the hop limit
    assert int((want_rows["fixed"] == rf.BOTH).sum()) >= 4000 and int((want_rows["fixed"] == abi.FIX_L4).sum()) >= 2000
    check(engine, batch, data, offs[:-1], [f for f, _ in got], want_rows, rf.to_set([rf.NAT44], incremental), None, "imix")


def test_the_65535_byte_frame(engine, corpus):
    i = [len(f) for f in corpus.garbage].index(65535)
    nat = rf.NAMES.index(rf.NAT44.name)
    for half in (corpus.fixed, corpus.garbage):
        out, rows = rf.ref_all(half, False)[nat]
        rows = rows.copy()
        rows["action"] = 0  # the set below holds this action alone
        assert int(rows[i]["fixed"]) == rf.BOTH
        frames = [half[i], half[0], half[i]]
        data, offs, lens, keep, batch = layout("packed", frames, 15)
        check(engine, batch, data, offs, [out[i], out[0], out[i]], rows[[i, 0, i]], rf.to_set([rf.NAT44]), None, "65535 B")


def test_two_runs_give_identical_buffers(engine, corpus):
    frames = [corpus.garbage[i] for i in rf.small(corpus.garbage)] * 4
    _, acts = rf.action_chunks()[0]
    index = _dev(np.arange(len(frames), dtype=np.uint8) % 17)
    for incremental in (False, True):
        res = []
        for _ in range(2):
            data, offs, lens, keep, batch = layout("offsets + lengths", frames, 7)
            rows = engine.rewrite(batch, rf.to_set(acts, incremental), index)
            res.append((batch.data.cpu().numpy(), rows.cpu().numpy()))
        assert (res[0][0] == res[1][0]).all() and (res[0][1] == res[1][1]).all()
        assert (res[0][0] != data).any()
