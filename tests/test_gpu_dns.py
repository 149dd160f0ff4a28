"""GPU: the DNS message pass (nexg_dns_batch, nexg_dns_entries) on hand-built
messages wrapped in Eth/IPv4/UDP and Eth/IPv6/UDP (tests/dns_frames.py).

Per batch: the nexg_dns array equals the generator's own expectation and
dns.dns_frame_host per frame (pinned by tests/test_dns_host.py), tile_first
equals the host prefix sums, every entry at tile_first[i >> 8] + first + k is
the expected one, and the names decoded from the entries' offsets are the
generator's. Shapes: the counts around a wave and a 256-frame tile, every
frame layout, 65,537 frames (the tile scan's second step), a capacity below the
total, tampered summaries, untrusted records. All comparisons are exact."""
import ctypes

import numpy as np
import pytest

from nex_amd import abi
from nex_amd import dns as hostdns
from nex_amd.engine import FrameBatch
from nex_amd.frame import ParseOption
from tests import dns_frames as df
from tests import helpers
from tests.helpers import layouts, to_host

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
VLAN = ParseOption(unwrap_vlan=True)
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def corpus():
    cases = df.cases()
    df.check_cases_against_host(cases)
    return cases


def run_dns(engine, batch, option=VLAN, **kw):
    import torch
    recs = engine.parse(batch, option, out_kind=abi.OUT_RECORD)
    dns, tile_first, entries, total = engine.dns(batch, recs, **kw)
    torch.cuda.synchronize()
    n = batch.count
    assert tile_first.numel() == (n + 255) // 256 + 1
    return (recs, dns, tile_first, entries, total, to_host(recs, abi.RECORD_DTYPE, n), to_host(dns, abi.DNS_DTYPE, n),
            tile_first.cpu().numpy().astype(np.uint64), to_host(entries, abi.DNS_ENTRY_DTYPE, entries.numel() // 16))


def expected(cs, port=53, any_udp=False, vlan_parsed=True):
    """(summaries with `first`, tile_first, per-frame entry lists) the
    generator's cases imply, prefix sums done on the host."""
    exp = [c.expect(port, any_udp, vlan_parsed) for c in cs]
    want = df.summary_array([s for s, _ in exp])
    k = np.array([len(e) for _, e in exp], np.int64)
    before = np.concatenate([[0], np.cumsum(k)])[: len(cs)]
    tiles = (len(cs) + 255) // 256
    tf = np.array([before[256 * t] for t in range(tiles)] + [int(k.sum())], np.uint64)
    if len(cs):
        want["first"] = before - tf[np.arange(len(cs)) >> 8].astype(np.int64)
    return want, tf, [e for _, e in exp]


def check(name, cs, frames, hrecs, hdns, htf, hent, total, port=53, any_udp=False, vlan_parsed=True):
    want, tf, per = expected(cs, port, any_udp, vlan_parsed)
    n = len(cs)
    assert len(hdns) == n, name
    assert (htf == tf).all() and int(total) == int(tf[-1]) == len(hent), (name, htf, tf, total)
    if not n:
        return
    helpers.records_equal(hdns, want, frames, f"{name}: summaries")
    for i, c in enumerate(cs):
        s, entries = hostdns.dns_frame_host(frames[i], hrecs[i], port, any_udp)  # summaries equal dns_host per frame
        for f in s:
            assert int(hdns[f][i]) == s[f], (name, i, c.what, f)
        base = int(htf[i >> 8]) + int(hdns["first"][i])
        rows = hent[base:base + len(per[i])]
        assert rows.tobytes() == df.entry_array(per[i]).tobytes() == df.entry_array(entries).tobytes(), (name, i, c.what)
        if per[i]:  # names decoded from the entries' offsets, out of the frame's own bytes
            mo, ml = int(hdns["msg_off"][i]), int(hdns["msg_len"][i])
            assert df.decoded_names(frames[i][mo:mo + ml], rows) == c.names, (name, i, c.what)
            pkt = hostdns.DnsPacket(frames[i], hdns[i], rows)
            assert [q.qname_parsed() for q in pkt.queries] == c.names, (name, i, c.what)
            assert (len(pkt.queries), len(pkt.responses), len(pkt.authorities), len(pkt.additionals)) == c.counts
            assert len(pkt.payload) == ml - c.rest_off, (name, i, c.what)


@pytest.mark.parametrize("count", COUNTS)
def test_dns_every_layout(engine, corpus, count):
    cs = df.cycled(corpus, count)
    frames = [c.frame for c in cs]
    for name, batch, _ in layouts(frames, strided_below=None):
        _, _, _, _, total, hrecs, hdns, htf, hent = run_dns(engine, batch)
        check(f"{name} n={count}", cs, frames, hrecs, hdns, htf, hent, total)
    if count >= 63:
        st = {int(s) for s in hdns["status"]}
        assert st == {abi.FRAME_OK, abi.ERR_BUFFER_TOO_SHORT, abi.ERR_MALFORMED}
        assert (hdns["flags8"] & abi.DNS_SECTION_SHORT).any() and (hent["flags8"] & abi.DNS_DATA_CUT).any()
        assert {int(s) for s in hent["section"]} == {0, 1, 2, 3}


def test_dns_options(engine, corpus):
    """NEXG_DNS_ANY_UDP, port 5353, port 0 = 53, and the batch parsed without
    the VLAN extension (the tagged query is then no UDP frame)."""
    cs = df.cycled(corpus, 257)
    frames = [c.frame for c in cs]
    batch = FrameBatch.from_packed(frames, pad_to=1, shift=4)
    seen = {}
    for kw in (dict(any_udp=True), dict(port=5353), dict(port=0), dict(port=5300), dict(port=5353, any_udp=True)):
        _, _, _, _, total, hrecs, hdns, htf, hent = run_dns(engine, batch, **kw)
        check(f"options {kw}", cs, frames, hrecs, hdns, htf, hent, total, kw.get("port", 53), kw.get("any_udp", False))
        seen[tuple(kw.items())] = {c.what for i, c in enumerate(cs) if hdns["flags8"][i] & abi.DNS_CANDIDATE}
    assert "udp to another port" in seen[(("any_udp", True),)] and "udp to 5353" in seen[(("any_udp", True),)]
    assert seen[(("port", 5353),)] == {"udp to 5353"} and seen[(("port", 5300),)] == {"udp to another port"}
    assert "udp to another port" not in seen[(("port", 0),)] and "reference query packet" in seen[(("port", 0),)]
    for option, vlan_parsed in ((VLAN, True), (ParseOption(), False)):
        _, _, _, _, total, hrecs, hdns, htf, hent = run_dns(engine, batch, option=option)
        check(f"vlan parsed {vlan_parsed}", cs, frames, hrecs, hdns, htf, hent, total, vlan_parsed=vlan_parsed)
        tagged = np.array([c.vlan for c in cs])
        assert tagged.any() and ((hdns["flags8"][tagged] & abi.DNS_CANDIDATE != 0) == vlan_parsed).all()


def test_dns_untrusted_records(engine, corpus):
    """A record whose payload reaches past its own frame (but stays inside the
    data tensor) makes the frame a non-candidate: all zero but `first`."""
    import torch
    cs = df.cycled(corpus, 65)
    frames = [c.frame for c in cs]
    batch = FrameBatch.from_packed(frames, pad_to=1, shift=4)
    _, _, _, _, total, hrecs, hdns, htf, hent = run_dns(engine, batch)
    victims = [i for i, c in enumerate(cs[:-1]) if c.entries and c.candidate()][:6]
    assert len(victims) == 6
    bad = hrecs.copy()
    for j, i in enumerate(victims):
        if j % 2:
            bad["payload_len"][i] += 1 + j
        else:
            bad["payload_off"][i] += bad["payload_len"][i] + j
        assert int(bad["payload_off"][i]) + int(bad["payload_len"][i]) > len(frames[i])
    dev = torch.from_numpy(bad.view(np.uint8).copy()).cuda()
    dns, tile_first, entries, total2 = engine.dns(batch, dev)
    torch.cuda.synchronize()
    d2 = to_host(dns, abi.DNS_DTYPE, 65)
    gone = sum(len(cs[i].entries) for i in victims)
    assert total2 == total - gone and int(tile_first[-1]) == total2
    keep = np.ones(65, bool)
    keep[victims] = False
    for i in victims:
        assert d2[i].tobytes()[:28] == bytes(28), i
    for f in abi.DNS_DTYPE.names:
        if f != "first":
            assert (d2[f][keep] == hdns[f][keep]).all(), f
    k = np.array([int(d2["n_q"][i]) + int(d2["n_an"][i]) + int(d2["n_ns"][i]) + int(d2["n_ar"][i]) for i in range(65)])
    assert (d2["first"] == np.concatenate([[0], np.cumsum(k)])[:65]).all()
    e2 = to_host(entries, abi.DNS_ENTRY_DTYPE, total2)
    assert e2.tobytes() == b"".join(df.entry_array(c.entries).tobytes() for i, c in enumerate(cs)
                                    if keep[i] and c.candidate() and c.status == abi.FRAME_OK)


def test_dns_65537_frames(engine):
    """256 x 256 + 1 two-entry frames: the tile scan crosses into its second
    256-tile step."""
    c = df.cases()[1]  # the reference's response packet: one query, one answer
    assert len(c.entries) == 2
    n = 65537
    stride = (len(c.frame) + 15) // 16 * 16
    a = np.zeros((n, stride), np.uint8)
    a[:, :len(c.frame)] = np.frombuffer(c.frame, np.uint8)
    batch = FrameBatch.from_strided(a, lengths=np.full(n, len(c.frame), np.int32))
    _, _, _, _, total, hrecs, hdns, htf, hent = run_dns(engine, batch)
    assert total == 2 * n and len(htf) == 258
    assert (htf == np.concatenate([np.arange(257, dtype=np.uint64) * 512, [2 * n]])).all()
    assert (hdns["first"] == (np.arange(n) % 256) * 2).all()
    want, _ = c.expect()
    for f, v in want.items():
        assert (hdns[f] == v).all(), f
    rows = df.entry_array(c.entries).tobytes()
    for i in (0, 255, 256, 65535, 65536):
        base = int(htf[i >> 8]) + int(hdns["first"][i])
        assert base == 2 * i and hent[base:base + 2].tobytes() == rows, i
    assert (hent["section"] == np.tile([0, 1], n)).all() and (hent["ttl"][1::2] == 900).all()


def _entries_call(engine, batch, dns_t, tf_t, buf, cap):
    fr = batch.to_c()
    P = ctypes.c_void_p
    return engine.lib.nexg_dns_entries(engine.ctx, ctypes.byref(fr), P(dns_t.data_ptr()), P(tf_t.data_ptr()),
                                       P(buf.data_ptr()), cap, None)


def test_entries_cap_below_total(engine, corpus):
    """Entries below the capacity are right, every byte at or past it keeps
    the sentinel, the total does not change."""
    import torch
    cs = df.cycled(corpus, 300)
    frames = [c.frame for c in cs]
    batch = FrameBatch.from_frames(frames, pad_to=4)
    _, dns, tile_first, entries, total, hrecs, hdns, htf, hent = run_dns(engine, batch)
    assert total > 200
    for cap in (0, 1, 7, total // 2, total - 1, total):
        buf = torch.full(((total + 8) * 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert _entries_call(engine, batch, dns, tile_first, buf, cap) == abi.OK
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert got[: cap * 16].tobytes() == hent[:cap].tobytes(), cap
        assert (got[cap * 16:] == SENTINEL).all(), cap
        assert (tile_first.cpu().numpy().astype(np.uint64) == htf).all() and int(tile_first[-1]) == total
    # Engine.dns with a capacity: no read-back, the same rows below it
    d2, tf2, e2, t2 = engine.dns(batch, engine.parse(batch, VLAN, out_kind=abi.OUT_RECORD), entries_cap=10)
    torch.cuda.synchronize()
    assert int(t2.item()) == total and e2.numel() == 160 and e2.cpu().numpy().tobytes() == hent[:10].tobytes()


def test_engine_dns_with_and_without_cap(engine, corpus):
    import torch
    cs = df.cycled(corpus, 257)
    batch = FrameBatch.from_packed([c.frame for c in cs], pad_to=1, shift=4)
    recs = engine.parse(batch, VLAN, out_kind=abi.OUT_RECORD)
    d1, tf1, e1, total = engine.dns(batch, recs)
    d2, tf2, e2, t2 = engine.dns(batch, recs, entries_cap=total)
    torch.cuda.synchronize()
    assert isinstance(total, int) and int(t2.item()) == total
    assert torch.equal(d1, d2) and torch.equal(tf1, tf2) and torch.equal(e1, e2) and e1.numel() == total * 16


def test_tampered_summaries_stay_inside_the_capacity(engine, corpus):
    """`first`, msg_len and the n_* counts overwritten with large values: the
    walk still reads only the frame's own bytes (msg_off + msg_len is clamped
    to the frame, every bound re-checked) and nothing at or past entries_cap is
    written; the call returns NEXG_OK. All memory involved is valid."""
    import torch
    cs = df.cycled(corpus, 300)
    frames = [c.frame for c in cs]
    batch = FrameBatch.from_frames(frames, pad_to=4)
    _, dns, tile_first, entries, total, hrecs, hdns, htf, hent = run_dns(engine, batch)
    for first, cap in ((None, 7), (0, 5), (0, total), (0xFFFFFFFF, 9), (3, 0)):
        bad = hdns.copy()
        if first is not None:
            bad["first"] = first
        bad["msg_len"] = 65535
        for f in ("n_q", "n_an", "n_ns", "n_ar"):
            bad[f] = 65535
        dev = torch.from_numpy(bad.view(np.uint8).copy()).cuda()
        buf = torch.full(((total + 64) * 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert _entries_call(engine, batch, dev, tile_first, buf, cap) == abi.OK
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[cap * 16:] == SENTINEL).all(), (first, cap)
        if first == 0xFFFFFFFF:
            assert (got == SENTINEL).all()
    assert torch.equal(to_dev_bytes(hdns), dns)  # the summaries themselves are inputs: untouched


def to_dev_bytes(a):
    import torch
    return torch.from_numpy(a.view(np.uint8).copy()).cuda()


def test_argument_errors(engine, corpus):
    """Every NEXG_EINVAL case returns -1 before any launch and leaves the
    outputs untouched; NULL entries with capacity 0 and an empty batch are
    valid."""
    import torch
    lib, ctx = engine.lib, engine.ctx
    frames = [c.frame for c in corpus[:8]]
    batch = FrameBatch.from_frames(frames)
    recs = engine.parse(batch, out_kind=abi.OUT_RECORD)
    n = batch.count
    out = torch.full((n * 32 + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    tf = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    ent = torch.full((64 * 16 + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    fr = batch.to_c()
    huge = abi.Frames(data=batch.data.data_ptr(), data_bytes=batch.data.numel(), offsets=None, lengths=None, stride=64,
                      hints=0, count=1 << 32)
    P = ctypes.c_void_p

    def walk(opt, o=out.data_ptr(), t=tf.data_ptr(), r=recs.data_ptr(), f=fr):
        return lib.nexg_dns_batch(ctx, ctypes.byref(f), P(r), None if opt is None else ctypes.byref(opt), P(o), P(t), None)

    def fill(d=out.data_ptr(), t=tf.data_ptr(), e=ent.data_ptr(), cap=64, f=fr):
        return lib.nexg_dns_entries(ctx, ctypes.byref(f), P(d), P(t), P(e), cap, None)

    assert abi.EINVAL == -1
    assert walk(abi.DnsOption(0, 0, 1)) == abi.EINVAL
    assert walk(abi.DnsOption(2, 0, 0)) == abi.EINVAL
    assert walk(abi.DnsOption(0x80000001, 53, 0)) == abi.EINVAL
    assert walk(None, o=None) == abi.EINVAL
    assert walk(None, t=None) == abi.EINVAL
    assert walk(None, r=None) == abi.EINVAL
    assert walk(None, o=out.data_ptr() + 8) == abi.EINVAL
    assert walk(None, t=tf.data_ptr() + 4) == abi.EINVAL
    assert walk(None, r=recs.data_ptr() + 8) == abi.EINVAL
    assert walk(None, f=huge) == abi.EINVAL
    assert fill(d=None) == abi.EINVAL
    assert fill(t=None) == abi.EINVAL
    assert fill(e=None) == abi.EINVAL
    assert fill(d=out.data_ptr() + 8) == abi.EINVAL
    assert fill(t=tf.data_ptr() + 4) == abi.EINVAL
    assert fill(e=ent.data_ptr() + 8) == abi.EINVAL
    assert fill(f=huge) == abi.EINVAL
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (tf == -1).all() and (ent == SENTINEL).all()
    # an empty batch writes tile_first[0] = 0 and nothing else
    empty = abi.Frames(data=None, data_bytes=0, offsets=None, lengths=None, stride=64, hints=0, count=0)
    assert walk(None, o=None, r=None, f=empty) == abi.OK
    assert fill(d=None, t=None, e=None, cap=0, f=empty) == abi.OK
    torch.cuda.synchronize()
    assert tf.tolist() == [0, -1, -1, -1] and (out == SENTINEL).all()
    # the valid calls
    assert walk(abi.DnsOption(abi.DNS_ANY_UDP, 0, 0)) == abi.OK
    assert walk(None) == abi.OK
    assert fill(e=None, cap=0) == abi.OK  # valid, launches nothing
    torch.cuda.synchronize()
    assert (ent == SENTINEL).all()
    total = int(tf[1])
    assert 0 < total <= 64 and fill() == abi.OK
    torch.cuda.synchronize()
    want = b"".join(df.entry_array(c.expect()[1]).tobytes() for c in corpus[:8])
    assert ent.cpu().numpy()[: total * 16].tobytes() == want and (ent[total * 16:] == SENTINEL).all()
    assert (out[n * 32:] == SENTINEL).all() and tf.tolist()[2:] == [-1, -1]
