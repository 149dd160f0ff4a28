"""GPU: tunnel decapsulation (nexg_decap_batch, nexg_decap_select) on known
inner frames wrapped in VXLAN / GRE outer headers (tests/tunnel_frames.py).

Per batch: the nexg_tunnel array, inner offsets and lengths equal
tunnel.decap_host per frame (pinned by tests/test_tunnel_host.py) and the
generator's own expectation; every accepted tunnel's inner bytes are the
wrapped frame; select + parse of each inner class equals the oracle's parse of
the wrapped frames. Shapes: the counts around a wave and a 256-frame tile, the
packed / offsets + lengths / fixed-stride / 32-bit-offset layouts, a tunnel
ending on the data tensor's last byte, a record reaching past its frame."""
import ctypes

import numpy as np
import pytest

from nex_amd import abi, tunnel
from nex_amd.engine import FrameBatch
from nex_amd.frame import ParseOption
from tests import helpers
from tests import tunnel_frames as tf
from tests.helpers import layouts, to_host

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
ETH = {abi.INNER_ETHERNET}
IP = {abi.INNER_IPV4, abi.INNER_IPV6}
VLAN = ParseOption(unwrap_vlan=True)
FROM_IP = ParseOption(from_ip_packet=True, offset=0)


@pytest.fixture(scope="module")
def corpus(oracle):
    """The case list and, per case, the oracle's record of the wrapped inner
    frame under the option its class is parsed with (computed once)."""
    cases = tf.cases()
    want = np.zeros(len(cases), abi.RECORD_DTYPE)
    for i, c in enumerate(cases):
        if c.inner is not None and c.inner_class == abi.INNER_ETHERNET:
            want[i] = oracle.parse_frame(c.inner)
        elif c.inner is not None and c.inner_class in IP:
            want[i] = oracle.parse_frame(c.inner, abi.PARSE_FROM_IP, 0)
    ids = {id(c): i for i, c in enumerate(cases)}
    return cases, want, ids


def outer_offsets(batch):
    if batch.offsets is None:
        return np.arange(batch.count, dtype=np.int64) * batch.stride
    return batch.host_offsets()[: batch.count]


def run_decap(engine, batch, option=VLAN, **kw):
    import torch
    recs = engine.parse(batch, option, out_kind=abi.OUT_RECORD)
    tunnels, inner = engine.decap(batch, recs, **kw)
    torch.cuda.synchronize()
    n = batch.count
    return (recs, tunnels, inner, to_host(recs, abi.RECORD_DTYPE, n), to_host(tunnels, abi.TUNNEL_DTYPE, n),
            to_host(inner.offsets, np.int64, n), to_host(inner.lengths, np.uint32, n))


def check_against_host(name, frames, batch, hrecs, htun, ioff, ilen, **kw):
    """1. tunnels, inner_off - off(i), inner_len == decap_host per frame."""
    host = [tunnel.decap_host(f, r, **kw) for f, r in zip(frames, hrecs)]
    assert len(htun) == len(ioff) == len(ilen) == len(frames), name
    if frames:
        helpers.records_equal(htun, tf.tunnels_array([h[0] for h in host]), frames, f"{name}: tunnels")
    off = outer_offsets(batch)
    assert (ioff - off == np.array([h[1] for h in host], np.int64)).all(), name
    assert (ilen == np.array([h[2] for h in host], np.uint32)).all(), name
    return host


def check_select_parse(engine, name, cs, corpus, batch, tunnels, inner, htun, ioff, ilen):
    """3. select + parse of each inner class == the oracle on the wrapped frames."""
    import torch
    _, want, ids = corpus
    assert inner.data.data_ptr() == batch.data.data_ptr() and inner.count == batch.count
    for classes, option in ((ETH, ParseOption()), (IP, FROM_IP)):
        idx, sel = engine.decap_select(tunnels, inner, classes)
        pick = np.nonzero((htun["kind"] != 0) & (htun["status"] == 0) & np.isin(htun["inner"], list(classes)))[0]
        assert sel.count == len(pick), (name, classes)
        assert (to_host(idx, np.uint32, sel.count) == pick).all(), (name, classes)
        assert (to_host(sel.offsets, np.int64, sel.count) == ioff[pick]).all(), (name, classes)
        assert (to_host(sel.lengths, np.uint32, sel.count) == ilen[pick]).all(), (name, classes)
        got = engine.parse_to_numpy(sel, option, out_kind=abi.OUT_RECORD)
        torch.cuda.synchronize()
        assert len(got) == len(pick), (name, classes)
        if len(pick):
            helpers.records_equal(got, want[[ids[id(cs[i])] for i in pick]], [cs[i].inner for i in pick],
                                  f"{name}: inner parse {sorted(classes)}")


@pytest.mark.parametrize("count", COUNTS)
def test_decap_every_layout(engine, corpus, count):
    cases = corpus[0]
    cs = tf.cycled(cases, count)
    frames = [c.frame for c in cs]
    for name, batch, _ in layouts(frames, strided_below=None):
        name = f"{name} n={count}"
        recs, tunnels, inner, hrecs, htun, ioff, ilen = run_decap(engine, batch)
        check_against_host(name, frames, batch, hrecs, htun, ioff, ilen)
        # the generator's own expectation, and 2. the inner bytes of every accepted tunnel
        data = batch.data.cpu().numpy()
        for i, c in enumerate(cs):
            assert (htun["kind"][i], htun["status"][i]) == (c.kind, c.status), (name, i, c.what)
            if c.inner is not None:
                assert htun["inner"][i] == c.inner_class, (name, i, c.what)
                assert data[ioff[i]:ioff[i] + ilen[i]].tobytes() == c.inner, (name, i, c.what)
            else:
                assert ilen[i] == 0, (name, i, c.what)
        if count and batch.offsets is not None and batch.lengths is None and batch.stride == 0:
            # tail: the last frame is a tunnel whose inner frame ends on the data tensor's final byte
            assert cs[-1].inner and ioff[-1] + ilen[-1] == batch.data.numel(), name
        monotone = batch.offsets is None or batch.lengths is None
        assert inner.hints == (abi.FRAMES_MONOTONE if monotone else 0), name
        check_select_parse(engine, name, cs, corpus, batch, tunnels, inner, htun, ioff, ilen)


def test_decap_options(engine, corpus):
    """One tunnel kind only, a custom VXLAN port, port 0 = 4789, and the outer
    batch parsed without the VLAN extension (tagged outer frames are then no
    tunnels): each equals decap_host under the same arguments."""
    cs = tf.cycled(corpus[0], 257)
    frames = [c.frame for c in cs]
    batch = FrameBatch.from_packed(frames, pad_to=1, shift=4)
    for kw in (dict(which=abi.DECAP_VXLAN), dict(which=abi.DECAP_GRE), dict(vxlan_port=4790), dict(vxlan_port=0),
               dict(which=0)):
        _, _, _, hrecs, htun, ioff, ilen = run_decap(engine, batch, **kw)
        check_against_host(f"options {kw}", frames, batch, hrecs, htun, ioff, ilen, **kw)
        which, port = kw.get("which", 3), kw.get("vxlan_port", 4789) or 4789
        for i, c in enumerate(cs):
            custom = c.what == "udp to 4790 (custom port)"
            k = (abi.TUN_VXLAN if custom else 0) if port == 4790 and c.kind != abi.TUN_GRE else c.kind
            k = k if which & (abi.DECAP_VXLAN if k == abi.TUN_VXLAN else abi.DECAP_GRE) else 0
            assert htun["kind"][i] == k, (kw, i, c.what)
    recs, tunnels, inner, hrecs, htun, ioff, ilen = run_decap(engine, batch, option=ParseOption())
    check_against_host("no vlan unwrap", frames, batch, hrecs, htun, ioff, ilen)
    tagged = np.array([c.vlan for c in cs])
    assert tagged.any() and (htun["kind"][tagged] == 0).all()
    assert (htun["kind"][~tagged] == np.array([c.kind for c in cs])[~tagged]).all()


def test_decap_clamps_untrusted_records(engine, corpus):
    """A record whose payload reaches past its own frame (but stays inside the
    data tensor) makes the frame a non-candidate: nothing outside the frame's
    extent decides the result."""
    import torch
    cs = tf.cycled(corpus[0], 65)
    frames = [c.frame for c in cs]
    batch = FrameBatch.from_packed(frames, pad_to=1, shift=4)
    recs, _, _, hrecs, htun, _, _ = run_decap(engine, batch)
    victims = [i for i, c in enumerate(cs[:-1]) if c.inner and c.kind in (abi.TUN_VXLAN, abi.TUN_GRE)][:6]
    assert {cs[i].kind for i in victims} == {abi.TUN_VXLAN, abi.TUN_GRE}
    bad = hrecs.copy()
    for j, i in enumerate(victims):
        assert htun["kind"][i] != 0
        if j % 2:
            bad["payload_len"][i] += 1 + j          # the payload runs into the next frame
        else:
            bad["payload_off"][i] += bad["payload_len"][i] + j  # the payload starts at / past the frame's end
        assert int(bad["payload_off"][i]) + int(bad["payload_len"][i]) > len(frames[i])
    dev = torch.from_numpy(bad.view(np.uint8).copy()).cuda()
    tunnels, inner = engine.decap(batch, dev)
    torch.cuda.synchronize()
    t2 = to_host(tunnels, abi.TUNNEL_DTYPE, 65)
    off = outer_offsets(batch)
    for i in victims:
        assert t2[i].tobytes() == bytes(16), i
        assert int(inner.offsets[i]) == off[i] and int(inner.lengths[i]) == 0
    keep = np.ones(65, bool)
    keep[victims] = False
    helpers.records_equal(t2[keep], htun[keep], None, "clamp: the other frames")


def synthetic(count, pattern, rng):
    t = np.zeros(count, abi.TUNNEL_DTYPE)
    t["kind"] = rng.integers(1, 3, count)
    t["inner"] = rng.integers(0, 4, count)
    t["status"] = 0
    if pattern == "none":
        t["status"][rng.random(count) < 0.5] = abi.ERR_MALFORMED
        t["kind"][t["status"] == 0] = 0
    elif pattern == "all":
        t["inner"] = rng.integers(1, 3, count)
    elif pattern == "alternating":
        t["inner"] = np.where(np.arange(count) % 2 == 0, 1, 3)
    else:  # random: every reason not to be selected
        t["status"][rng.random(count) < 0.2] = abi.ERR_MALFORMED
        t["kind"][rng.random(count) < 0.2] = 0
    off = rng.integers(0, 1 << 40, count).astype(np.int64)
    ln = rng.integers(0, 65536, count).astype(np.uint32)
    return t, off, ln


@pytest.mark.parametrize("count", [1, 256, 257, 65793])
def test_select_alone(engine, count):
    """nexg_decap_select on synthetic arrays against numpy: none, all,
    alternating and random selections; 65,793 frames are 257 tiles + 1 frame,
    so the tile scan crosses its own 256-wide chunk."""
    import torch
    rng = np.random.default_rng(count)
    for pattern in ("none", "all", "alternating", "random"):
        t, off, ln = synthetic(count, pattern, rng)
        inner = FrameBatch(data=torch.zeros(16, dtype=torch.uint8, device="cuda"), count=count,
                           offsets=torch.from_numpy(off).cuda(), lengths=torch.from_numpy(ln.view(np.int32)).cuda())
        dt = torch.from_numpy(t.view(np.uint8).copy()).cuda()
        for classes in ({1, 2}, {3}, {0, 1, 2, 3}):
            idx, sel = engine.decap_select(dt, inner, classes)
            pick = np.nonzero((t["kind"] != 0) & (t["status"] == 0) & np.isin(t["inner"], list(classes)))[0]
            what = (count, pattern, classes)
            assert sel.count == len(pick), what
            assert (to_host(idx, np.uint32, sel.count) == pick).all(), what
            assert (to_host(sel.offsets, np.int64, sel.count) == off[pick]).all(), what
            assert (to_host(sel.lengths, np.uint32, sel.count) == ln[pick]).all(), what
        if pattern == "none":
            assert len(pick) == 0
        if pattern == "all":
            assert len(pick) == count


def test_argument_errors(engine):
    """NEXG_EINVAL before any launch: reserved != 0, unknown `which` bits, NULL
    and misaligned outputs, a short workspace, too many frames; count 0 is ok."""
    import torch
    lib, ctx = engine.lib, engine.ctx
    frames = [c.frame for c in tf.cases()[:8]]
    batch = FrameBatch.from_frames(frames)
    recs = engine.parse(batch, out_kind=abi.OUT_RECORD)
    n = batch.count
    tun = torch.zeros(n * 16 + 16, dtype=torch.uint8, device="cuda")
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    ln = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    fr = batch.to_c()
    P = ctypes.c_void_p

    def decap(opt, t=tun.data_ptr(), o=off.data_ptr(), l=ln.data_ptr(), r=recs.data_ptr(), f=fr):
        return lib.nexg_decap_batch(ctx, ctypes.byref(f), P(r), None if opt is None else ctypes.byref(opt), P(t), P(o),
                                    P(l), None)

    assert decap(abi.DecapOption(3, 0, 0)) == abi.OK
    assert decap(None) == abi.OK
    assert decap(abi.DecapOption(3, 0, 1)) == abi.EINVAL
    assert decap(abi.DecapOption(4, 0, 0)) == abi.EINVAL
    assert decap(abi.DecapOption(7, 4789, 0)) == abi.EINVAL
    assert decap(None, t=tun.data_ptr() + 8) == abi.EINVAL
    assert decap(None, o=off.data_ptr() + 4) == abi.EINVAL
    assert decap(None, l=ln.data_ptr() + 2) == abi.EINVAL
    assert decap(None, t=None) == abi.EINVAL
    assert decap(None, r=None) == abi.EINVAL
    empty = abi.Frames(data=None, data_bytes=0, offsets=None, lengths=None, stride=64, hints=0, count=0)
    assert decap(None, t=None, o=None, l=None, r=None, f=empty) == abi.OK

    oi = torch.zeros(n, dtype=torch.int32, device="cuda")
    oo = torch.zeros(n, dtype=torch.int64, device="cuda")
    ol = torch.zeros(n, dtype=torch.int32, device="cuda")
    cnt = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    need = abi.decap_select_workspace(n)
    ws = torch.zeros(need + 8, dtype=torch.uint8, device="cuda")

    def select(count=n, wsb=need, w=ws.data_ptr(), c=cnt.data_ptr(), t=tun.data_ptr(), i=oi.data_ptr()):
        return lib.nexg_decap_select(ctx, P(t), P(off.data_ptr()), P(ln.data_ptr()), count, 0xE, P(i), P(oo.data_ptr()),
                                     P(ol.data_ptr()), P(c), P(w), wsb, None)

    assert select() == abi.OK
    assert select(wsb=need - 1) == abi.EINVAL
    assert select(wsb=0) == abi.EINVAL
    assert select(w=None) == abi.EINVAL
    assert select(w=ws.data_ptr() + 2) == abi.EINVAL
    assert select(c=None) == abi.EINVAL
    assert select(c=cnt.data_ptr() + 4) == abi.EINVAL
    assert select(t=tun.data_ptr() + 8) == abi.EINVAL
    assert select(i=oi.data_ptr() + 2) == abi.EINVAL
    assert select(count=1 << 32, wsb=1 << 40) == abi.EINVAL
    torch.cuda.synchronize()
    assert int(cnt[1]) == -1
    assert select(count=0, wsb=0, w=None) == abi.OK  # nothing selected: only the count is written
    torch.cuda.synchronize()
    assert int(cnt[0]) == 0
