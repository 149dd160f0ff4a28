"""GPU: frame selection by rule (nexg_select_batch) on the explicit corpus of
tests/select_frames.py.

The expectation is nex_amd.select.match_host (pinned by the hand-derived truth
table in tests/test_select_host.py) applied to the oracle's records of the
corpus, computed once per filter and tiled to each count: out_index, out_off,
out_len, out_rule and *out_count must equal it for every table rule and
multi-rule filter. Shapes: the counts around a wave, a 256-frame tile and the
scan's 256-tile carry (65793 = 258 tiles); the packed / offsets + lengths /
fixed-stride / 32-bit-offset layouts; records that point past their frame;
select composed with parse, decap, gather_rows and dns."""
import ctypes

import numpy as np
import pytest

from nex_amd import abi
from nex_amd import select as S
from nex_amd.engine import FrameBatch
from nex_amd.frame import ParseMode, ParseOption
from nex_amd.select import Filter, Rule
from tests import helpers
from tests import select_frames as sf
from tests.helpers import layouts, parse_records, to_host

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1000, 65793]
VLAN = ParseOption(unwrap_vlan=True)
#: the filters run on every layout (all of them run on the first layout)
EVERY_LAYOUT = ("tcp syn to 10/8", "port 53 any", "src net 2001:db8::/32", "v6 src X/33", "length 60-65",
                "issue examples", "sixteen", "inverted v6")


class Corpus:
    """The corpus, the oracle's records, and match_host's verdict per frame
    for a filter (computed once per filter, cached by name)."""

    def __init__(self, oracle):
        self.items = sf.corpus()
        self.frames = [x.frame for x in self.items]
        self.recs = oracle.parse_frames(self.frames, sf.PARSE_FLAGS)
        self.cache = {}

    def verdicts(self, name, flt):
        if name not in self.cache:
            v = [S.match_host(f, r, len(f), flt) for f, r in zip(self.frames, self.recs)]
            self.cache[name] = (np.array([x[0] for x in v], bool), np.array([x[1] for x in v], np.uint8))
        return self.cache[name]

    def tiled(self, count):
        which = np.arange(count) % len(self.frames)
        return which, [self.frames[i] for i in which]


@pytest.fixture(scope="module")
def corp(oracle):
    return Corpus(oracle)


def table_of(batch):
    """Host (offsets, lengths) of a batch as its table defines them."""
    if batch.offsets is None:
        off = np.arange(batch.count, dtype=np.int64) * batch.stride
    else:
        off = batch.host_offsets()[: batch.count]
    return off, batch.frame_lengths()


def check_select(engine, name, batch, recs, flt, want_sel, want_rule):
    idx, sel, rule = engine.select(batch, recs, flt, want_rule=True)
    pick = np.nonzero(want_sel)[0]
    off, ln = table_of(batch)
    assert sel.count == len(pick), (name, sel.count, len(pick))
    assert (to_host(idx, np.uint32, sel.count) == pick).all(), name
    assert (to_host(sel.offsets, np.int64, sel.count) == off[pick]).all(), name
    assert (to_host(sel.lengths, np.uint32, sel.count) == ln[pick]).all(), name
    assert (to_host(rule, np.uint8, sel.count) == want_rule[pick]).all(), name
    assert sel.data.data_ptr() == batch.data.data_ptr()
    return idx, sel


@pytest.mark.parametrize("count", COUNTS)
def test_select_parity_every_layout(engine, corp, count):
    which, frames = corp.tiled(count)
    filters = sf.all_filters()
    for li, (lname, batch, keep) in enumerate(layouts(frames, only_first=count > 1000)):
        w = which if keep is None else which[keep]
        recs = parse_records(engine, batch)
        if count in (65, 1000) and li == 0:  # the device records are the oracle's (the expectation's input)
            helpers.records_equal(to_host(recs, abi.RECORD_DTYPE, count), corp.recs[which], frames, "records")
        for fname, flt in filters:
            if li and fname not in EVERY_LAYOUT:
                continue
            sel, rule = corp.verdicts(fname, flt)
            check_select(engine, f"{lname} n={count} {fname}", batch, recs, flt, sel[w], rule[w])


def test_select_is_deterministic(engine, corp):
    import torch
    which, frames = corp.tiled(65793)
    batch = FrameBatch.from_packed(frames, pad_to=1)
    recs = parse_records(engine, batch)
    for fname in ("issue examples", "inverted v6"):
        runs = []
        for _ in range(2):
            idx, sel, rule = engine.select(batch, recs, sf.FILTERS[fname], want_rule=True)
            runs.append((idx.clone(), sel.offsets.clone(), sel.lengths.clone(), rule.clone()))
        assert 0 < len(runs[0][0]) < 65793
        for a, b in zip(*runs):
            assert torch.equal(a, b), fname


def _raw_select(engine, batch, recs, fc, idx, off, ln, rule, cnt, ws, ws_bytes):
    fr = batch.to_c()
    p = lambda t: None if t is None else ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())  # noqa: E731
    return engine.lib.nexg_select_batch(engine.ctx, ctypes.byref(fr), p(recs), None if fc is None else ctypes.byref(fc),
                                        p(idx), p(off), p(ln), p(rule), p(cnt), p(ws), ws_bytes, engine._stream(None))


def test_pointer_level_rejections(engine, corp):
    import torch
    _, frames = corp.tiled(300)
    batch = FrameBatch.from_packed(frames, pad_to=1)
    recs = parse_records(engine, batch)
    n = batch.count
    fc = Filter([Rule.udp()]).to_c()
    idx = torch.zeros(n + 4, dtype=torch.int32, device="cuda")
    off = torch.zeros(n + 4, dtype=torch.int64, device="cuda")
    ln = torch.zeros(n + 4, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    wsb = abi.select_workspace(n)
    ws = torch.zeros(wsb + 8, dtype=torch.uint8, device="cuda")
    good = dict(recs=recs, fc=fc, idx=idx, off=off, ln=ln, rule=None, cnt=cnt, ws=ws, ws_bytes=wsb)
    assert _raw_select(engine, batch, **good) == abi.OK
    torch.cuda.synchronize()
    assert int(cnt[0]) == int(corp.verdicts("udp", Filter([Rule.udp()]))[0][np.arange(n) % len(corp.frames)].sum())
    for key in ("recs", "fc", "idx", "off", "ln", "cnt", "ws"):
        assert _raw_select(engine, batch, **dict(good, **{key: None})) == abi.EINVAL, key
    for key, t, step in (("off", off, 4), ("idx", idx, 2), ("ln", ln, 1), ("cnt", cnt, 4), ("ws", ws, 2), ("recs", recs, 8)):
        assert _raw_select(engine, batch, **dict(good, **{key: t.data_ptr() + step})) == abi.EINVAL, key
    assert _raw_select(engine, batch, **dict(good, ws_bytes=wsb - 1)) == abi.EINVAL
    bad = Filter([Rule(tests=abi.RULE_SRC_PORT, sport_lo=2, sport_hi=1)]).to_c(validate=False)
    assert _raw_select(engine, batch, **dict(good, fc=bad)) == abi.EINVAL
    assert b"sport_lo > sport_hi" in engine.lib.nexg_ctx_last_error(engine.ctx)
    with pytest.raises(ValueError):
        engine.select(batch, recs, Filter([]))
    # count == 0 writes *out_count = 0 and needs nothing else
    empty = FrameBatch.from_packed([], pad_to=1)
    cnt.fill_(7)
    assert _raw_select(engine, empty, None, fc, None, None, None, None, cnt, None, 0) == abi.OK
    torch.cuda.synchronize()
    assert int(cnt[0]) == 0


def test_hostile_records(engine, corp):
    """Records are caller memory: l3_off past the frame, and an IPv6 header
    that would end on the data tensor's last byte. Nothing faults and the
    verdict is match_host's on the same records."""
    import torch
    base = [f for f in corp.frames if len(f) < 2000]
    v6 = next(x.frame for x in corp.items if x.what == "v6 udp to 53")
    frames = (base * 5)[:299] + [v6]  # the last frame ends on the data tensor's last byte
    batch = FrameBatch.from_packed(frames, pad_to=1)
    assert batch.data.numel() == sum(len(f) for f in frames)
    recs = parse_records(engine, batch)
    torch.cuda.synchronize()
    h = to_host(recs, abi.RECORD_DTYPE, len(frames))
    rng = np.random.default_rng(5)
    for i in range(len(frames)):
        k = i % 6
        if k == 1:
            h["l3_off"][i] = len(frames[i]) + int(rng.integers(0, 3))       # at or just past the end
        elif k == 2:
            h["l3_off"][i] = 65535
        elif k == 3:
            h["l3_off"][i] = max(0, len(frames[i]) - 40 + int(rng.integers(-1, 2)))  # header ends at the frame end +-1
        elif k == 4:
            h["flags"][i] = int(h["flags"][i]) | abi.L_IPV6                 # claims a layer the frame lacks
    last = len(frames) - 1
    h["l3_off"][last] = len(v6) - 40  # ends exactly on the last byte of the data
    h["flags"][last] = abi.L_ETHERNET | abi.L_IP | abi.L_IPV6
    dev = torch.from_numpy(h.view(np.uint8).copy()).cuda()
    tail = v6[len(v6) - 32:]
    filters = [("all v6", Filter([Rule.net("::/0", "src")])), ("db8 src", sf.FILTERS["issue examples"]),
               ("tail src", Filter([Rule(tests=abi.RULE_SRC_ADDR, family=6, src=tail[:16], src_bits=128)])),
               ("tail dst", Filter([Rule(tests=abi.RULE_DST_ADDR, family=6, dst=tail[16:], dst_bits=128)])),
               ("inverted", sf.FILTERS["inverted v6"])]
    for name, flt in filters:
        v = [S.match_host(f, r, len(f), flt) for f, r in zip(frames, h)]
        sel, rule = np.array([x[0] for x in v], bool), np.array([x[1] for x in v], np.uint8)
        check_select(engine, f"hostile {name}", batch, dev, flt, sel, rule)
        if name.startswith("tail"):
            assert sel[last]  # the address bytes were read from the very end of the data


def test_parse_of_the_selected_table(engine, corp):
    which, frames = corp.tiled(600)
    batch = FrameBatch.from_packed(frames, pad_to=1)
    recs = parse_records(engine, batch)
    flt = sf.FILTERS["issue examples"]
    sel, rule = corp.verdicts("issue examples", flt)
    idx, tab = check_select(engine, "compose parse", batch, recs, flt, sel[which], rule[which])
    got = engine.parse_to_numpy(tab, VLAN, ParseMode.Strict, out_kind=abi.OUT_RECORD)
    pick = np.nonzero(sel[which])[0]
    helpers.records_equal(got, corp.recs[which][pick], [frames[i] for i in pick], "parse(selected)")
    rows = engine.gather_rows(recs, 64, idx)
    helpers.records_equal(to_host(rows, abi.RECORD_DTYPE, len(pick)), corp.recs[which][pick], None, "gather_rows")


def test_select_on_a_decap_inner_table(engine, oracle):
    """The pass works unchanged on an inner table with the inner records."""
    from tests import tunnel_frames as tf
    cs = tf.cycled(tf.cases(), 300)
    batch = FrameBatch.from_packed([c.frame for c in cs], pad_to=1)
    recs = engine.parse(batch, VLAN, out_kind=abi.OUT_RECORD)
    tunnels, inner = engine.decap(batch, recs)
    oidx, eth = engine.decap_select(tunnels, inner, {abi.INNER_ETHERNET})
    rec_eth = engine.parse(eth, out_kind=abi.OUT_RECORD)
    wrapped = [cs[i].inner for i in to_host(oidx, np.uint32, eth.count)]
    assert len(wrapped) > 50 and all(w is not None for w in wrapped)
    want_recs = oracle.parse_frames(wrapped)
    for name, flt in (("tcp", Filter([Rule.tcp()])), ("udp or v6", Filter([Rule.udp(), Rule.net("::/0")])),
                      ("short", Filter([Rule.length(0, 60)], invert=True))):
        v = [S.match_host(f, r, len(f), flt) for f, r in zip(wrapped, want_recs)]
        sel, rule = np.array([x[0] for x in v], bool), np.array([x[1] for x in v], np.uint8)
        assert 0 < sel.sum() < len(sel), name
        check_select(engine, f"inner {name}", eth, rec_eth, flt, sel, rule)


def test_gather_rows_then_dns_on_the_selected_table(engine):
    """gather_rows(records, index) + Engine.dns on the selected table equals
    the full-batch DNS summaries at index."""
    import torch
    from tests import dns_frames as df
    cs = df.cycled(df.cases(), 700)
    batch = FrameBatch.from_packed([c.frame for c in cs], pad_to=1)
    recs = engine.parse(batch, VLAN, out_kind=abi.OUT_RECORD)
    full, _, _, total = engine.dns(batch, recs)
    idx, sel = engine.select(batch, recs, Filter([Rule.udp() & Rule.port(53)]))
    assert 0 < sel.count < batch.count
    rec_sel = engine.gather_rows(recs, 64, idx)
    part, _, _, total_sel = engine.dns(sel, rec_sel)
    torch.cuda.synchronize()
    hfull = to_host(full, abi.DNS_DTYPE, batch.count)
    hpart = to_host(part, abi.DNS_DTYPE, sel.count)
    pick = to_host(idx, np.uint32, sel.count)
    for n in abi.DNS_DTYPE.names:
        if n != "first":  # the entry position inside the frame's own tile
            assert (hpart[n] == hfull[n][pick]).all(), n
    assert (hfull["flags8"] & abi.DNS_CANDIDATE).sum() == (hpart["flags8"] & abi.DNS_CANDIDATE).sum() > 0
    assert total_sel == total
    # the other row sizes' use: the summaries themselves compact the same way
    rows = engine.gather_rows(full, 32, idx)
    assert to_host(rows, abi.DNS_DTYPE, sel.count).tobytes() == hfull[pick].tobytes()
