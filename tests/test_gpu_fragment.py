"""GPU: IPv4 fragmentation to an MTU (nexg_fragment_plan, nexg_fragment_frames;
Engine.fragment).

Every output byte, pads included, the output table (offsets, lengths, source
index) and the rows must equal nex_amd.fragment.fragment_host exactly (which
tests/test_fragment_host.py pins from outside). Shapes: the corpus of
tests/fragment_frames.py in every table form of tests.helpers.layouts (sources
at every byte phase), mtu 68 / 576 / 1500, align 1 and 16; input counts around
a workgroup of the fill (16 frames), a plan tile (256) and 4097; a frame of
8183 pieces last in one workgroup and first in the next; a destination
pre-filled with 0xA5, a capacity that cuts a frame, first / bytes tables that
lie, two runs; encap -> fragment -> parse, reassembled and decapsulated on the
way back; a per-frame row carried to the pieces by Engine.gather_rows."""
import ctypes
import functools

import numpy as np
import pytest

from nex_amd import abi
from nex_amd.encap import Tunnel, TunnelSet, encap_host
from nex_amd.engine import FrameBatch
from nex_amd.fragment import FragOption, fragment_frame, plan_host
from tests import fragment_frames as ff
from tests import helpers

pytestmark = pytest.mark.gpu

FILL = 0xA5
COUNTS = (1, 15, 16, 17, 255, 256, 257, 4097)


@functools.lru_cache(maxsize=None)
def per_frame(mtu, ignore_df):
    """fragment_frame of every corpus frame, once per option."""
    return [fragment_frame(f, mtu, ignore_df) for f in ff.frames()]


def host(ids, mtu, ignore_df):
    """fragment_host over the corpus frames `ids` (indices, in table order), from per_frame."""
    cache = per_frame(mtu, ignore_df)
    pieces, src = [], []
    rows = np.zeros(len(ids), abi.FRAGGED_DTYPE)
    for i, c in enumerate(ids):
        p, status, kind, hl, pd = cache[c]
        rows[i] = (status, kind, hl, 0, len(p), pd, len(pieces), 0)
        pieces += p
        src += [i] * len(p)
    return pieces, np.array(src, np.uint32), rows


def want_buffer(pieces, align):
    offs = plan_host([len(p) for p in pieces], align)
    buf = np.zeros(int(offs[-1]), np.uint8)
    for o, p in zip(offs[:-1], pieces):
        buf[o:o + len(p)] = np.frombuffer(p, np.uint8)
    return offs, buf


def check_fragment(engine, name, batch, want, mtu, ignore_df, align):
    """Engine.fragment of `batch` against (pieces, src, rows)."""
    import torch
    pieces, src, rows = want
    out, d_src, d_rows = engine.fragment(batch, mtu, ignore_df, align)
    torch.cuda.synchronize()
    offs, buf = want_buffer(pieces, align)
    assert out.count == len(pieces) and out.data.numel() == len(buf), (name, out.count, len(pieces), out.data.numel(), len(buf))
    got_rows = helpers.to_host(d_rows, abi.FRAGGED_DTYPE, batch.count)
    bad = np.nonzero(got_rows.view(np.uint8).reshape(-1, 16) != rows.view(np.uint8).reshape(-1, 16))[0]
    assert len(bad) == 0, (name, int(bad[0]), got_rows[bad[0]], rows[bad[0]])
    assert (out.offsets.cpu().numpy() == offs).all(), name
    assert d_src.dtype == torch.int32 and (d_src.cpu().numpy().view(np.uint32) == src).all(), name
    if align == 1:
        assert out.lengths is None
    else:
        assert (out.lengths.cpu().numpy() == [len(p) for p in pieces]).all(), name
        assert out.hints == abi.FRAMES_MONOTONE
    got = out.data.cpu().numpy()
    if not (got == buf).all():
        b = int(np.nonzero(got != buf)[0][0])
        k = int(np.searchsorted(offs, b, side="right")) - 1
        raise AssertionError(f"{name}: byte {b} (output frame {k} of input {src[k]}, at {b - int(offs[k])} of {len(pieces[k])}) "
                             f"is {got[b]}, want {buf[b]}")
    return out, d_src, d_rows


@pytest.mark.parametrize("align,ignore_df", ((1, False), (16, True)))
@pytest.mark.parametrize("mtu", (68, 576, 1500))
def test_corpus_in_every_table_form(engine, mtu, align, ignore_df):
    ids = [i for i, f in enumerate(ff.frames()) if f is not None]
    frames = [ff.frames()[i] for i in ids]
    forms = set()
    for name, batch, keep in helpers.layouts(frames, strided_below=4096):
        sub = ids if keep is None else [ids[i] for i in keep]
        check_fragment(engine, f"mtu {mtu} align {align} {name}", batch, host(sub, mtu, ignore_df), mtu, ignore_df, align)
        forms.add((batch.offsets is None, batch.lengths is None, bool(batch.hints & abi.FRAMES_OFFSETS32)))
    # fixed stride, packed u64, offsets + lengths, and both u32 tables
    assert forms >= {(True, False, False), (False, True, False), (False, False, False), (False, True, True), (False, False, True)}


@pytest.mark.parametrize("align", (1, 16))
def test_extents_that_leave_the_data(engine, align):
    """Rule 1 on the device: an offset past the data, an extent that ends past
    it, a length over 65535: no output frame, NEXG_ERR_BAD_EXTENT."""
    ids = ff.small(2100)
    ids = [i for i in ids if ff.frames()[i] is not None]
    batch = FrameBatch.from_frames([ff.frames()[i] for i in ids])
    nbytes = batch.data.numel()
    boff, blen = batch.offsets.clone(), batch.lengths.clone()
    gone = next(i for i, (name, _) in enumerate(ff.corpus()) if name == "bad extent")
    ids = list(ids)
    for n, k in enumerate(range(3, len(ids), 11)):
        kind = n % 5
        if kind == 0:
            boff[k] = nbytes + 1
        elif kind == 1:
            boff[k] = (1 << 62) + 5
        elif kind == 2:
            blen[k] = 65536
        elif kind == 3:
            blen[k] = -1  # 0xFFFFFFFF
        else:
            boff[k], blen[k] = nbytes - 7, 8  # ends one byte past the data
        ids[k] = gone
    want = host(ids, 576, False)
    assert int((want[2]["status"] == abi.ERR_BAD_EXTENT).sum()) >= 5  # each of the five ways once
    for hints in (0, abi.FRAMES_MONOTONE):
        bad = FrameBatch(data=batch.data, count=batch.count, offsets=boff, lengths=blen, hints=hints)
        check_fragment(engine, f"bad extents align {align} hints {hints}", bad, want, 576, False, align)


@pytest.mark.parametrize("align", (1, 16))
@pytest.mark.parametrize("count", COUNTS)
def test_counts(engine, count, align):
    """The group and tile edges of both kernels: 16 input frames per workgroup
    of the fill, 256 per tile of the plan; 4097 is 17 tiles and a frame."""
    small = [i for i in ff.small(2100) if ff.frames()[i] is not None]
    ids = [small[(i + 3) % len(small)] for i in range(count)]
    batch = helpers.packed_from_byte_1([ff.frames()[i] for i in ids])
    want = host(ids, 576, align == 16)
    if count >= 255:
        assert len(want[0]) > count and int((want[2]["kind"] == abi.FRAG_TOO_BIG).sum()) > 0
    check_fragment(engine, f"n={count} align {align}", batch, want, 576, align == 16, align)


def test_a_many_piece_frame_last_in_a_workgroup_and_first_in_the_next(engine):
    big = next(i for i, (name, _) in enumerate(ff.corpus()) if name == "65535 bytes, hl 60")
    small = [i for i in ff.small(600) if ff.frames()[i] is not None]
    ids = [small[i % len(small)] for i in range(33)]
    ids[15] = ids[16] = big
    want = host(ids, 68, False)
    assert want[2]["pieces"][15] == want[2]["pieces"][16] == 8183
    batch = FrameBatch.from_packed([ff.frames()[i] for i in ids], pad_to=1, shift=4)
    check_fragment(engine, "8183 pieces twice", batch, want, 68, False, 1)
    check_fragment(engine, "8183 pieces twice, align 16", batch, want, 68, False, 16)


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def raw_plan(engine, batch, oc, first, nbytes, rows):
    import torch
    ws_bytes = abi.fragment_plan_workspace(batch.count)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    fr = batch.to_c()
    rc = engine.lib.nexg_fragment_plan(engine.ctx, ctypes.byref(fr), ctypes.byref(oc), P(first), P(nbytes), P(rows), P(ws), ws_bytes,
                                       engine._stream(None))
    assert rc == abi.OK, engine.lib.nexg_ctx_last_error(engine.ctx)


def raw_frames(engine, batch, oc, first, nbytes, out_count, offs, ln, src, out, cap):
    fr = batch.to_c()
    rc = engine.lib.nexg_fragment_frames(engine.ctx, ctypes.byref(fr), ctypes.byref(oc), P(first), P(nbytes), out_count, P(offs), P(ln),
                                         P(src), P(out), cap, engine._stream(None))
    assert rc == abi.OK, engine.lib.nexg_ctx_last_error(engine.ctx)


@functools.lru_cache(maxsize=None)
def table_257():
    small = [i for i in ff.small(3500) if ff.frames()[i] is not None]
    return tuple(small[(i + 11) % len(small)] for i in range(257))


@pytest.mark.parametrize("align", (1, 16))
def test_prefilled_destination_out_cap_and_two_runs(engine, align):
    """Nothing is stored outside the frames' ranges or at or past out_cap, the
    pads are zero, the table has no entry past out_count, and a second run gives
    the same bytes."""
    import torch
    ids = table_257()
    n = len(ids)
    pieces, src, rows = host(ids, 576, False)
    batch = helpers.packed_from_byte_1([ff.frames()[i] for i in ids])
    oc = FragOption(576, 0, align).to_c()
    offs, buf = want_buffer(pieces, align)
    total, k = len(buf), len(pieces)
    first = torch.full((n + 3,), -1, dtype=torch.int32, device="cuda")
    nbytes = torch.full((n + 3,), -1, dtype=torch.int64, device="cuda")
    d_rows = torch.full(((n + 2) * 16,), FILL, dtype=torch.uint8, device="cuda")
    raw_plan(engine, batch, oc, first, nbytes, d_rows)
    torch.cuda.synchronize()
    hf, hb = first.cpu().numpy(), nbytes.cpu().numpy()
    assert (hf[:n] == rows["first"]).all() and hf[n] == k and (hf[n + 1:] == -1).all()
    first_of = np.concatenate([rows["first"].astype(np.int64), [k]])
    assert (hb[:n + 1] == offs[first_of]).all() and (hb[n + 1:] == -1).all()
    r = d_rows.cpu().numpy()
    assert (r[n * 16:] == FILL).all() and (r[: n * 16].view(abi.FRAGGED_DTYPE) == rows).all()
    # a cut in the middle of a split frame's second piece, in a pass-through frame, in a header, and none at all
    split = next(i for i in range(100, n) if rows["pieces"][i] >= 3)
    passed = next(i for i in range(150, n) if rows["kind"][i] == abi.FRAG_PASS and len(pieces[rows["first"][i]]) > 40)
    caps = (total, int(offs[rows["first"][split] + 1]) + 301, int(offs[rows["first"][passed]]) + 23,
            int(offs[rows["first"][split] + 2]) + 16, 5, 0)
    runs = []
    for cap in caps:
        out = torch.full((total + 4096,), FILL, dtype=torch.uint8, device="cuda")
        t_off = torch.full((k + 3,), -1, dtype=torch.int64, device="cuda")
        t_len = torch.full((k + 2,), -1, dtype=torch.int32, device="cuda")
        t_src = torch.full((k + 2,), -1, dtype=torch.int32, device="cuda")
        raw_frames(engine, batch, oc, first, nbytes, k, t_off, t_len, t_src, out, cap)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[cap:] == FILL).all(), (align, cap, "a store at or past out_cap")
        assert (got[:cap] == buf[:cap]).all(), (align, cap)
        # the table does not depend on the capacity
        assert (t_off.cpu().numpy()[: k + 1] == offs).all() and (t_off.cpu().numpy()[k + 1:] == -1).all(), cap
        assert (t_len.cpu().numpy()[:k] == [len(p) for p in pieces]).all() and (t_len.cpu().numpy()[k:] == -1).all(), cap
        assert (t_src.cpu().numpy()[:k].view(np.uint32) == src).all() and (t_src.cpu().numpy()[k:] == -1).all(), cap
        if cap == total:
            runs.append(got)
    out = torch.full((total + 4096,), FILL, dtype=torch.uint8, device="cuda")
    raw_frames(engine, batch, oc, first, nbytes, k, t_off, t_len, t_src, out, total)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == runs[0]).all()


def test_wrong_first_and_bytes_store_nothing_outside_a_frames_range(engine):
    """out_first and out_bytes are caller memory: ranges that shrink, run
    backwards or start past the capacity never move a byte store outside
    [out_bytes[i], out_bytes[i + 1]) or past out_cap; a first[i + 1] below the
    frame's pieces, or an out_count below them, ends its table entries there."""
    import torch
    ids = table_257()[:64]
    n = len(ids)
    pieces, src, rows = host(ids, 576, False)
    batch = FrameBatch.from_frames([ff.frames()[i] for i in ids])
    oc = FragOption(576, 0, 1).to_c()
    offs, buf = want_buffer(pieces, 1)
    total, k = len(buf), len(pieces)
    first_of = np.concatenate([rows["first"].astype(np.int64), [k]])
    byte_of = offs[first_of]
    multi = []
    for i in range(2, n - 2):  # four frames of three pieces and more, no two of them neighbours' neighbours
        if rows["pieces"][i] >= 3 and (not multi or i >= multi[-1] + 3):
            multi.append(i)
    a, b, c, d = multi[:4]
    bad_b = byte_of.copy()
    bad_b[a] = bad_b[a + 1]                       # frame a has no room at all
    bad_b[b + 1] = byte_of[b] + 700               # frame b's room ends in its second piece (frame b + 1 starts early)
    bad_b[c] = total + 100000                     # frame c starts past the capacity
    bad_f = first_of.copy()
    bad_f[d + 1] = first_of[d] + 1                # frame d may write one table entry (frame d + 1 writes over the next)
    out = torch.full((total + 4096,), FILL, dtype=torch.uint8, device="cuda")
    t_off = torch.full((k + 3,), -1, dtype=torch.int64, device="cuda")
    t_len = torch.full((k + 2,), -1, dtype=torch.int32, device="cuda")
    t_src = torch.full((k + 2,), -1, dtype=torch.int32, device="cuda")
    cut = k - 2                                   # out_count two below the table: the last frame's last entries stay out
    raw_frames(engine, batch, oc, torch.from_numpy(bad_f.astype(np.int32)).cuda(), torch.from_numpy(bad_b).cuda(), cut, t_off, t_len,
               t_src, out, total)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[total:] == FILL).all()
    touched = {a - 1, a, b, b + 1, c - 1, c}      # a frame in front of a moved start may zero up to 15 pad bytes less
    for i in range(n):
        if i not in touched:
            assert got[byte_of[i]:byte_of[i + 1]].tobytes() == buf[byte_of[i]:byte_of[i + 1]].tobytes(), i
    for i in (a, c):  # nothing of its own; the frame in front, given its room, may zero up to 15 pad bytes of it
        assert (got[byte_of[i] + 15:byte_of[i + 1]] == FILL).all(), i
        assert np.isin(got[byte_of[i]:byte_of[i] + 15], (0, FILL)).all(), i
    assert got[byte_of[b]:byte_of[b] + 700].tobytes() == buf[byte_of[b]:byte_of[b] + 700].tobytes()
    h_off, h_len, h_src = t_off.cpu().numpy(), t_len.cpu().numpy(), t_src.cpu().numpy()
    assert (h_len[cut:] == -1).all() and (h_src[cut:] == -1).all() and (h_off[cut + 1:] == -1).all()
    assert h_off[cut] == bad_b[n]                 # out_offsets[out_count] = out_bytes[count]
    assert h_src[first_of[d]] == d and h_len[first_of[d]] == len(pieces[first_of[d]])
    for f in range(first_of[d] + 1, first_of[d + 1]):  # frame d's later entries: left alone, or frame d + 1's (its first is moved)
        assert h_src[f] in (-1, d + 1), f
    ok = [f for f in range(cut) if src[f] not in (a, b + 1, c, d, d + 1)]
    assert (h_src[ok].view(np.uint32) == src[ok]).all() and (h_len[ok] == np.array([len(pieces[f]) for f in ok])).all()


@functools.lru_cache(maxsize=None)
def vtep():
    return TunnelSet([Tunnel.vxlan(vni=5001, src="10.0.0.1", dst="10.0.0.2", eth_dst="02:00:00:00:00:02",
                                   eth_src="02:00:00:00:00:01", src_port=49152, udp_csum=True, ip_id=0x4242)])


def test_encap_then_fragment_then_parse_and_back(engine, oracle):
    """A tunnel endpoint on a 1500-byte link: VXLAN puts 50 bytes in front of
    every frame, the 1500-byte class no longer fits and leaves as two pieces.
    Every piece parses with an OK IPv4 header checksum; the pieces, reassembled
    on the host and decapsulated on the device, give the inner frames back."""
    import torch
    inner = [oracle.gen_frame(abi.WL_IMIX, i) for i in range(300)]
    assert max(len(f) for f in inner) >= 1500
    want_outer, _ = encap_host(inner, vtep())
    outer, _ = engine.encap(FrameBatch.from_packed(inner, pad_to=1), vtep())
    out, d_src, d_rows = engine.fragment(outer, 1500)
    torch.cuda.synchronize()
    rows = helpers.to_host(d_rows, abi.FRAGGED_DTYPE, len(inner))
    n_split = int((rows["kind"] == abi.FRAG_SPLIT).sum())
    assert n_split == sum(len(f) + 36 > 1500 for f in inner) > 0 and (rows["pieces"][rows["kind"] == abi.FRAG_SPLIT] == 2).all()
    assert ((rows["kind"] == abi.FRAG_PASS) | (rows["kind"] == abi.FRAG_SPLIT)).all()
    # the output is a packed batch the parse takes as it stands
    rec = engine.parse_to_numpy(out, out_kind=abi.OUT_RECORD)
    assert out.count == len(inner) + n_split == len(rec)
    assert ((rec["flags"] & abi.L_IPV4) != 0).all() and ((rec["flags"] & abi.C_IP_OK) != 0).all()
    assert (rec["ip_length"] <= 1500).all()
    data, offs, src = out.data.cpu().numpy(), out.offsets.cpu().numpy(), d_src.cpu().numpy()
    pieces = [data[offs[f]:offs[f + 1]].tobytes() for f in range(out.count)]
    back = []
    for i in range(len(inner)):
        mine = [pieces[f] for f in np.nonzero(src == i)[0]]
        assert len(mine) == rows["pieces"][i]
        back.append(mine[0] if rows["kind"][i] == abi.FRAG_PASS else ff.reassemble(mine))
    assert back == want_outer
    again = FrameBatch.from_packed(back, pad_to=1)
    rec2 = engine.parse(again, out_kind=abi.OUT_RECORD)
    tun, tab = engine.decap(again, rec2)
    th = helpers.to_host(tun, abi.TUNNEL_DTYPE, len(inner))
    assert (th["kind"] == abi.TUN_VXLAN).all() and (th["status"] == 0).all() and (th["id"] == 5001).all()
    d2, o2, l2 = again.data.cpu().numpy(), tab.offsets.cpu().numpy(), tab.lengths.cpu().numpy()
    for i, f in enumerate(inner):
        assert d2[o2[i]:o2[i] + l2[i]].tobytes() == f, i


def test_gather_rows_carries_a_per_frame_row_to_the_pieces(engine):
    import torch
    ids = table_257()
    pieces, src, rows = host(ids, 576, True)
    batch = FrameBatch.from_frames([ff.frames()[i] for i in ids], pad_to=4)
    out, d_src, _ = engine.fragment(batch, 576, ignore_df=True, report=False)
    rule = (np.arange(len(ids), dtype=np.uint32) * 2654435761 + 17).astype(np.uint32)
    got = engine.gather_rows(torch.from_numpy(rule.view(np.int32)).cuda(), 4, d_src)
    torch.cuda.synchronize()
    assert out.count == len(pieces) > len(ids)
    assert (helpers.to_host(got, np.uint32, len(pieces)) == rule[src]).all()
