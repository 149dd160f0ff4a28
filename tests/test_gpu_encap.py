"""GPU: tunnel encapsulation (nexg_encap_plan, nexg_encap_frames; Engine.encap).

Offsets, lengths, rows and every output byte, pads included, must equal
nex_amd.encap.encap_host exactly (which tests/test_encap_host.py pins to the
oracle's builders). Shapes: the counts around a quarter wave's workgroup (16
frames), a wave, a 256-frame plan tile and the scan's 256-tile carry; every
layout of tests.helpers.layouts (sources at every byte phase); align 1 and 16
(destinations at every byte phase); every spec of tests/encap_frames.py; inner
lengths from 0 to the longest that fits; an output capacity that cuts a frame;
a canary behind the total; two runs; the round trip through the parse and
decap kernels; a tunnel index from Engine.select; source ports from
Engine.flow; the far batch's frames around 2 GiB and 4 GiB."""
import ctypes
import functools

import numpy as np
import pytest

from nex_amd import abi
from nex_amd import select as S
from nex_amd.encap import TunnelSet, encap_host, plan_host
from nex_amd.engine import FrameBatch
from nex_amd.frame import ParseMode, ParseOption
from tests import encap_frames as ef
from tests import helpers

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
VLAN = ParseOption(unwrap_vlan=True)
CANARY = 0xC7


def dev_u8(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def want_buffer(frames, align):
    offs = plan_host([len(f) for f in frames], align)
    buf = np.zeros(int(offs[-1]), np.uint8)
    for o, f in zip(offs[:-1], frames):
        buf[o:o + len(f)] = np.frombuffer(f, np.uint8)
    return offs, buf


def check_encap(engine, name, batch, want, want_rows, tunnels, index, flows, align):
    """Engine.encap of `batch` against the expected outer frames and rows."""
    import torch
    ti = None if index is None else dev_u8(np.asarray(index, np.uint8))
    fl = None if flows is None else dev_u8(flows)
    out, rows = engine.encap(batch, tunnels, ti, fl, align)
    torch.cuda.synchronize()
    n = batch.count
    offs, buf = want_buffer(want, align)
    assert out.count == n and out.data.numel() == len(buf), (name, out.data.numel(), len(buf))
    assert (out.offsets.cpu().numpy() == offs).all(), name
    if align == 1:
        assert out.lengths is None
    else:
        assert (out.lengths.cpu().numpy() == [len(w) for w in want]).all(), name
        assert out.hints == abi.FRAMES_MONOTONE
    got_rows = helpers.to_host(rows, abi.ENCAPPED_DTYPE, n)
    bad = [i for i in range(n) if ef.row_tuple(got_rows[i]) != ef.row_tuple(want_rows[i])]
    assert not bad, (name, bad[0], got_rows[bad[0]], want_rows[bad[0]])
    got = out.data.cpu().numpy()
    if not (got == buf).all():
        b = int(np.nonzero(got != buf)[0][0])
        k = int(np.searchsorted(offs, b, side="right")) - 1
        raise AssertionError(f"{name}: byte {b} (frame {k}, at {b - int(offs[k])} of {len(want[k])}, tunnel "
                             f"{None if index is None else index[k]}) is {got[b]}, want {buf[b]}")
    return out, rows


@functools.lru_cache(maxsize=None)
def table(count, which):
    """`count` inner frames, their tunnel numbers and flow rows under spec set
    `which`, and what encap_host makes of them."""
    tunnels, numbers = ef.spec_sets()[which]
    inner = list(ef.small_inner())
    frames = [inner[(i * 7 + which + 1) % len(inner)] for i in range(count)]  # (a batch of one frame is not an empty one)
    for i in range(5, count, 97):
        frames[i] = bytes(range(1, 13)) + b"\x08\x00" + ef.pattern(1486 + i % 3, i)
    if count >= 255:  # the longest inner frame that fits spec 0 of the set, and one byte more
        frames[100], frames[200] = ef.limit_inner(ef.specs()[numbers[0]])
    index = [i % (len(numbers) + 2) if i % 19 else abi.TUNNEL_NONE for i in range(count)]
    if count >= 255:
        index[100] = index[200] = 0
    flows = ef.flows_array(ef.hashes_for(count, seed=count + which))
    want, rows = encap_host(frames, tunnels, index, flows)
    return tunnels, frames, index, flows, want, rows


@pytest.mark.parametrize("align", (1, 16))
@pytest.mark.parametrize("count", COUNTS)
def test_counts_layouts_and_specs(engine, count, align):
    for which in (0, 1):
        tunnels, frames, index, flows, want, rows = table(count, which)
        for name, batch, keep in helpers.layouts(frames, only_first=which == 1 and count > 0):
            if keep is None:
                check_encap(engine, f"n={count} set {which} {name} align {align}", batch, want, rows, tunnels, index, flows, align)
            else:  # the strided batch leaves the long frames out: the sequence numbers follow the table
                w, r = encap_host([frames[i] for i in keep], tunnels, [index[i] for i in keep], flows[keep])
                check_encap(engine, f"n={count} set {which} {name} align {align}", batch, w, r, tunnels,
                            [index[i] for i in keep], flows[keep], align)


def test_no_index_and_no_report(engine):
    tunnels = TunnelSet([ef.specs()[2]])
    frames = list(ef.small_inner())
    want, rows = encap_host(frames, tunnels)
    batch = FrameBatch.from_packed(frames, pad_to=1)
    check_encap(engine, "no index", batch, want, rows, tunnels, None, None, 4)
    out, none = engine.encap(batch, tunnels, report=False)
    assert none is None and out.data.cpu().numpy().tobytes() == b"".join(want)
    # an index or flow rows of the wrong kind, place or size are refused before any call
    import torch
    n = len(frames)
    flow_set = TunnelSet([ef.specs()[1]])
    for kw in (dict(index=torch.zeros(n, dtype=torch.int32, device="cuda")), dict(index=torch.zeros(n - 1, dtype=torch.uint8, device="cuda")),
               dict(index=torch.zeros(n, dtype=torch.uint8)), dict(flows=torch.zeros(n * 8 - 1, dtype=torch.uint8, device="cuda")),
               dict(flows=torch.zeros(n * 8, dtype=torch.uint8)), dict(flows=None), dict(align=2)):
        with pytest.raises(ValueError):
            engine.encap(batch, flow_set, **dict(dict(flows=torch.zeros(n * 8, dtype=torch.uint8, device="cuda")), **kw))


def raw_frames(engine, batch, tc, index, flows, offs, out, cap, rows):
    fr = batch.to_c()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = engine.lib.nexg_encap_frames(engine.ctx, ctypes.byref(fr), ctypes.byref(tc), p(index), p(flows), p(offs), p(out), cap,
                                      p(rows), engine._stream(None))
    assert rc == abi.OK, engine.lib.nexg_ctx_last_error(engine.ctx)


@pytest.mark.parametrize("align", (1, 16))
def test_canary_out_cap_and_two_runs(engine, align):
    import torch
    tunnels, frames, index, flows, want, rows = table(257, 0)
    batch = helpers.packed_from_byte_1(frames)
    offs, buf = want_buffer(want, align)
    total = len(buf)
    d_offs = torch.from_numpy(offs).cuda()
    ti, fl, tc = dev_u8(np.asarray(index, np.uint8)), dev_u8(flows), tunnels.to_c()
    # a frame cut by out_cap: a 1500-B one in the middle of the table, and the header of the one after the longest
    k = next(i for i in range(120, 257) if len(want[i]) > 1400)
    runs = []
    for cap in (total, int(offs[k]) + 700, int(offs[101]) + 23, int(offs[k]) + 16, 5, 0):
        out = torch.full((total + 4096,), CANARY, dtype=torch.uint8, device="cuda")
        d_rows = torch.full(((257 + 2) * 8,), CANARY, dtype=torch.uint8, device="cuda")
        raw_frames(engine, batch, tc, ti, fl, d_offs, out, cap, d_rows)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[cap:] == CANARY).all(), (align, cap, "a store at or past out_cap")
        cut = np.searchsorted(offs, cap, side="right") - 1  # the frame that holds byte `cap`
        whole = int(offs[min(cut, 257)])
        assert (got[:whole] == buf[:whole]).all(), (align, cap)
        if cap < total and cap > whole:  # the cut frame's bytes below the cap, but for a checksum over a part of it
            a, b = got[whole:cap].copy(), buf[whole:cap].copy()
            if rows[cut]["l4_csum"]:
                at = int(rows[cut]["hdr_len"]) - 10
                a[at:at + 2] = b[at:at + 2] = 0
            assert (a == b).all(), (align, cap, int(cut))
        r = d_rows.cpu().numpy()
        assert (r[257 * 8:] == CANARY).all()
        if cap == total:
            assert (r[: 257 * 8].view(abi.ENCAPPED_DTYPE) == rows).all()
            runs.append(got)
    # the same call again: bit for bit
    out = torch.full((total + 4096,), CANARY, dtype=torch.uint8, device="cuda")
    raw_frames(engine, batch, tc, ti, fl, d_offs, out, total, None)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == runs[0]).all()


def test_wrong_offsets_store_nothing_outside_a_frames_range(engine):
    """out_offsets is caller memory: offsets that shrink, run backwards or
    point past the capacity never move a store outside [out_offsets[i],
    out_offsets[i + 1]) or past out_cap, and room given to a frame whose extent
    leaves the data is zeroed (15 bytes of it) without a read of its source."""
    import torch
    tunnels, frames, index, flows, want, rows = table(64, 0)
    batch = FrameBatch.from_frames(frames)
    # two frames with room at a start that is no multiple of 16 lose their extent: an offset far past the data, and
    # a length over 65535
    used = {9, 10, 11, 19, 20, 21, 29, 30, 31, 39, 40, 41}
    free = [k for k in range(1, 63) if len(want[k]) > 20 and not {k - 1, k, k + 1} & used]
    gone = [free[0], next(k for k in free if k > free[0] + 2)]
    boff, blen = batch.offsets.clone(), batch.lengths.clone()
    boff[gone[0]] = (1 << 45) + 3
    blen[gone[1]] = 70000
    batch = FrameBatch(data=batch.data, count=batch.count, offsets=boff, lengths=blen)
    offs, buf = want_buffer(want, 1)
    total = len(buf)
    assert all(int(offs[k]) % 16 for k in gone)
    bad = offs.copy()
    bad[10] = bad[11]                  # frame 10 has no room at all
    bad[20] = bad[21] - 5              # frame 20 has 5 bytes
    bad[30] = total + 100000           # frame 30 starts past the capacity
    bad[40], bad[41] = offs[41], offs[40]  # 40 runs backwards; 39 reaches over 40's room, 41 starts early
    out = torch.full((total + 4096,), CANARY, dtype=torch.uint8, device="cuda")
    d_rows = torch.full((64 * 8,), CANARY, dtype=torch.uint8, device="cuda")
    raw_frames(engine, batch, tunnels.to_c(), dev_u8(np.asarray(index, np.uint8)), dev_u8(flows), torch.from_numpy(bad).cuda(),
               out, total, d_rows)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[total:] == CANARY).all()
    for i in (0, 9, 11, 19, 21, 29, 31, 63, gone[0] - 1, gone[0] + 1, gone[1] - 1, gone[1] + 1):  # frames whose own range is intact are whole
        assert got[offs[i]:offs[i + 1]].tobytes() == want[i], i
    hrows = d_rows.cpu().numpy().view(abi.ENCAPPED_DTYPE)
    for k in gone:  # 15 pad bytes of the room, nothing else; status and the tunnel number in the row
        assert (got[offs[k]:offs[k] + 15] == 0).all() and (got[offs[k] + 15:offs[k + 1]] == CANARY).all(), k
        assert ef.row_tuple(hrows[k]) == (abi.ERR_BAD_EXTENT, index[k], 0, 0, 0, 0), (k, hrows[k])
    # a frame without room stores nothing; the frame before it may zero up to 15 pad bytes of the room it was given
    for k, end in ((10, int(offs[11])), (20, int(offs[21]) - 5), (30, int(offs[31]))):
        assert (got[int(offs[k]) + 15:end] == CANARY).all(), k
        assert np.isin(got[int(offs[k]):min(int(offs[k]) + 15, end)], (0, CANARY)).all(), k
    if len(want[20]) >= 5:
        assert got[offs[21] - 5:offs[21]].tobytes() == want[20][:5]


@pytest.mark.parametrize("align", (1, 16))
def test_extents_that_leave_the_data(engine, align):
    """Rule 1 on the device: an offset past the data, an extent that ends past
    it, a length over 65535: length 0, NEXG_ERR_BAD_EXTENT, and the frame's
    tunnel number in the row, also a number past the set."""
    tunnels, frames, index, flows, _, _ = table(256, 0)
    frames, index = list(frames), list(index)
    batch = FrameBatch.from_frames(frames)
    nbytes = batch.data.numel()
    boff, blen = batch.offsets.clone(), batch.lengths.clone()
    for n, k in enumerate(range(3, 256, 11)):
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
        frames[k] = None
        index[k] = (0, 5, 15, 16, 77, abi.TUNNEL_NONE)[n % 6]
    bad = FrameBatch(data=batch.data, count=batch.count, offsets=boff, lengths=blen)
    want, rows = encap_host(frames, tunnels, index, flows)
    assert int((rows["status"] == abi.ERR_BAD_EXTENT).sum()) == 23
    assert {int(t) for t in rows["tunnel"][rows["status"] == abi.ERR_BAD_EXTENT]} == {0, 5, 15, 16, 77, abi.TUNNEL_NONE}
    check_encap(engine, f"bad extents align {align}", bad, want, rows, tunnels, index, flows, align)
    check_encap(engine, f"bad extents monotone hint align {align}",
                FrameBatch(data=bad.data, count=bad.count, offsets=boff, lengths=blen, hints=abi.FRAMES_MONOTONE), want, rows,
                tunnels, index, flows, align)


def records_of(oracle, frames):
    return oracle.parse_frames(frames, abi.PARSE_VLAN)


@pytest.mark.parametrize("which", (0, 1))
def test_round_trip_through_parse_and_decap(engine, oracle, which):
    tunnels, numbers = ef.spec_sets()[which]
    ports = {(t.dst_port or abi.VXLAN_PORT) for t in tunnels.tunnels if t.kind == abi.ENCAP_VXLAN} or {abi.VXLAN_PORT}
    inner = [f for f in ef.small_inner()]
    for j, k in enumerate(numbers):
        t = ef.specs()[k]
        flows = ef.flows_array(ef.hashes_for(len(inner)))
        want, rows = encap_host(inner, tunnels, [j] * len(inner), flows)
        batch = FrameBatch.from_packed(inner, pad_to=1)
        outer, drows = check_encap(engine, f"spec {k}", batch, want, rows, tunnels, [j] * len(inner), flows, 1)
        rec = engine.parse(outer, VLAN, out_kind=abi.OUT_RECORD)
        got = helpers.to_host(rec, abi.RECORD_DTYPE, len(inner))
        helpers.records_equal(got, records_of(oracle, want), want, f"spec {k}: outer records")
        ok = rows["status"] == abi.FRAME_OK
        if t.family == 4:
            assert ((got["flags"][ok] & abi.C_IP_OK) != 0).all(), k
        if t.flags & abi.ENCAP_UDP_CSUM:
            assert ((got["flags"][ok] & abi.C_L4_OK) != 0).all(), k
        port = t.dst_port or abi.VXLAN_PORT
        tun, inner_table = engine.decap(outer, rec, vxlan_port=port)
        th = helpers.to_host(tun, abi.TUNNEL_DTYPE, len(inner))
        assert (th["kind"][ok] == t.kind).all() and (th["status"][ok] == 0).all(), k
        if t.l3_mode:
            continue  # the inner table holds IP packets and whatever else followed the dropped header: compared as bytes
        idx, eth = engine.decap_select(tun, inner_table, {abi.INNER_ETHERNET})
        picked = helpers.to_host(idx, np.uint32, idx.numel())
        assert picked.tolist() == np.nonzero(ok)[0].tolist(), k
        back = engine.parse_to_numpy(eth, VLAN, out_kind=abi.OUT_RECORD)
        helpers.records_equal(back, records_of(oracle, [inner[i] for i in picked]), None, f"spec {k}: inner records")
    assert ports


def test_l3_inner_bytes_come_back(engine, oracle):
    t = ef.specs()[8 + 7]  # GRE over IPv4, key, sequence, L3
    assert t.l3_mode and t.family == 4
    tunnels = TunnelSet([t])
    inner = [f for f in ef.small_inner() if len(f) >= 14]
    want, rows = encap_host(inner, tunnels)
    batch = FrameBatch.from_frames(inner)
    outer, _ = check_encap(engine, "l3", batch, want, rows, tunnels, None, None, 8)
    rec = engine.parse(outer, VLAN, out_kind=abi.OUT_RECORD)
    tun, tab = engine.decap(outer, rec)
    th = helpers.to_host(tun, abi.TUNNEL_DTYPE, len(inner))
    off, ln = tab.offsets.cpu().numpy(), tab.lengths.cpu().numpy()
    data = outer.data.cpu().numpy()
    for i, f in enumerate(inner):
        assert th["proto"][i] == int.from_bytes(f[12:14], "big") and th["aux"][i] == (t.seq_base + i) % (1 << 32)
        assert data[off[i]:off[i] + ln[i]].tobytes() == f[14:], i


def test_tunnel_by_rule_from_select(engine, oracle):
    """A match-action table: 16 rules, 16 tunnels; rule j gets tunnel j, and
    the index values 16, 77 and NEXG_TUNNEL_NONE pass a frame through."""
    import torch
    from tests import select_frames as sf
    frames = [x.frame for x in sf.cycled(sf.small_corpus(), 600)]
    batch = FrameBatch.from_packed(frames, pad_to=1)
    rec = helpers.parse_records(engine, batch)
    # 16 rules by length band, so every rule has frames
    edges = sorted({len(f) for f in frames})
    bands = [0] + [edges[i * len(edges) // 16] for i in range(1, 16)] + [65536]
    flt = S.Filter([S.Rule.length(bands[i], bands[i + 1] - 1) for i in range(16)])
    idx, sel, rule = engine.select(batch, rec, flt, want_rule=True)
    picked = helpers.to_host(idx, np.uint32, idx.numel())
    rules = helpers.to_host(rule, np.uint8, rule.numel())
    assert len(set(rules.tolist())) >= 8
    tunnels = ef.spec_sets()[0][0]
    flows = engine.flow(sel, engine.gather_rows(rec, 64, idx))
    hflows = helpers.to_host(flows, abi.FLOW_DTYPE, sel.count)
    inner = [frames[i] for i in picked]
    want, rows = encap_host(inner, tunnels, rules, hflows)
    check_encap(engine, "by rule", sel, want, rows, tunnels, rules, hflows, 1)
    # the same table under an index with the three ways to say "no tunnel"
    mixed = rules.copy()
    mixed[1::5], mixed[2::5], mixed[3::5] = abi.TUNNEL_NONE, 16, 77
    want, rows = encap_host(inner, tunnels, mixed, hflows)
    assert int((rows["tunnel"] == abi.TUNNEL_NONE).sum()) >= 3 * (len(inner) // 5)
    check_encap(engine, "mixed index", sel, want, rows, tunnels, mixed, hflows, 16)


def test_flow_port_from_engine_flow(engine, oracle):
    """RFC 7348's entropy: the source port follows the inner flow's hash, so
    one inner flow keeps one outer port and the flows spread over the span."""
    frames = [oracle.gen_frame(abi.WL_IMIX, i) for i in range(512)]
    frames += frames[:64]  # the same flows again: the same ports again
    batch = FrameBatch.from_packed(frames, pad_to=1)
    rec = engine.parse(batch, out_kind=abi.OUT_RECORD)
    flows = engine.flow(batch, rec)
    hflows = helpers.to_host(flows, abi.FLOW_DTYPE, len(frames))
    tunnels = TunnelSet([ef.specs()[3], ef.specs()[7]])  # UDP_CSUM + FLOW_PORT over IPv4 and IPv6
    index = [i % 2 for i in range(len(frames))]
    want, rows = encap_host(frames, tunnels, index, hflows)
    import torch
    out, drows = engine.encap(batch, tunnels, dev_u8(np.asarray(index, np.uint8)), flows)
    torch.cuda.synchronize()
    got = helpers.to_host(drows, abi.ENCAPPED_DTYPE, len(frames))
    assert (got == rows).all()
    assert out.data.cpu().numpy().tobytes() == b"".join(want)
    assert (got["src_port"][:64] == got["src_port"][512:]).all() and len(set(got["src_port"].tolist())) > 100
    orec = engine.parse_to_numpy(out, out_kind=abi.OUT_RECORD)
    assert ((orec["flags"] & abi.C_L4_OK) != 0).all() and (orec["src_port"] == got["src_port"]).all()


def test_65793_short_frames(engine, oracle):
    """257 plan tiles + 1 frame: the tile scan crosses its own 256-tile chunk."""
    import torch
    batch = engine.gen_batch(abi.WL_UDP64, 65793)
    assert batch.stride == 64 and batch.offsets is None
    t = ef.specs()[2]  # VXLAN over IPv4 with the UDP checksum
    tunnels = TunnelSet([t])
    out, rows = engine.encap(batch, tunnels, align=16)
    torch.cuda.synchronize()
    n, H = 65793, t.header_len()
    assert (out.offsets.cpu().numpy() == np.arange(n + 1, dtype=np.int64) * 128).all()
    assert (out.lengths.cpu().numpy() == H + 64).all()
    got = out.data.cpu().numpy().reshape(n, 128)
    raw = batch.data.cpu().numpy().reshape(n, 64)
    assert (got[:, H:H + 64] == raw).all() and (got[:, H + 64:] == 0).all()
    hr = helpers.to_host(rows, abi.ENCAPPED_DTYPE, n)
    for i in (0, 1, 255, 256, 257, 65535, 65536, 65791, 65792):
        w, r = encap_host([raw[i].tobytes()], tunnels)
        assert got[i, :H + 64].tobytes() == w[0] and ef.row_tuple(hr[i]) == ef.row_tuple(r[0]), i
    rec = engine.parse_to_numpy(out, out_kind=abi.OUT_RECORD)
    assert ((rec["flags"] & (abi.C_IP_OK | abi.C_L4_OK)) == (abi.C_IP_OK | abi.C_L4_OK)).all()


def test_far_batch_frames_around_2_and_4_gib(engine, oracle):
    """The far batch (tests/far_batch.py, placed as tests/test_gpu_far_batch.py
    places it): the frames around byte 2^31 and byte 2^32 of the buffer, through
    u64 offsets + lengths and through the u32 table with group bases. Source
    addresses at and above 2^32, and a frame that straddles each boundary."""
    import torch
    from tests import far_batch as fb
    from tests.test_gpu_far_batch import Device
    try:
        buf = torch.zeros(fb.BUFFER_BYTES, dtype=torch.uint8, device="cuda")
    except RuntimeError as e:  # torch.OutOfMemoryError is one
        pytest.skip(f"a {fb.BUFFER_BYTES}-B device allocation was refused: {e}")
    try:
        dev = Device(buf)
        pl = dev.place("A")
        # one 256-frame group of the u32 table: every frame within 4 GiB of the group's first, as the table's contract asks
        rows = sorted({r for b in fb.BOUNDARIES for r in range(pl.row[b] - 40, pl.row[b] + 40)})
        off, ln, ids = pl.off[rows], pl.length[rows], pl.ids[rows]
        for b in fb.BOUNDARIES:
            assert ((off < b) & (off + ln > b)).any() and (off >= b).any(), b
        frames = [dev.far.frames[i] for i in ids]
        n = len(rows)
        index = [(r % 18) if r % 18 < 17 else abi.TUNNEL_NONE for r in range(n)]
        flows = ef.flows_array(ef.hashes_for(n, seed=31))
        tunnels = ef.spec_sets()[0][0]
        want, wrows = encap_host(frames, tunnels, index, flows)
        assert int((wrows["status"] == abi.FRAME_OK).sum()) > n // 2
        b64 = FrameBatch(data=buf, count=n, offsets=torch.from_numpy(off).cuda(),
                         lengths=torch.from_numpy(ln.astype(np.int32)).cuda())
        b32 = b64.with_offsets32()
        assert b32.offsets.numel() == abi.offsets32_layout(n, True)[3]
        for name, batch, align in (("u64 offsets", b64, 16), ("u32 offsets with bases", b32, 1)):
            check_encap(engine, f"far A {name}", batch, want, wrows, tunnels, index, flows, align)
    finally:
        del buf
        torch.cuda.empty_cache()
