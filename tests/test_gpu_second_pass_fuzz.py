"""GPU: randomised differential sweeps of the four second passes
(nexg_dns_batch / nexg_dns_entries, nexg_decap_batch / nexg_decap_select,
nexg_select_batch, nexg_flow_batch / nexg_flow_partition) on the fuzz corpus
of tests/second_pass_fuzz.py, compared exactly with the independent references
of tests/second_pass_ref.py (not only with the host contracts, which
tests/test_second_pass_ref.py shows equal to them on the same corpus).

The kernels are one lane per frame, so content decides, not count: each sweep
is one shuffled batch of 5083 frames (19 whole 256-frame tiles with uneven
totals and 4 whole 1024-frame partition tiles, each followed by a ragged one),
in two layouts: packed from byte 1 (every alignment for the byte walks and the
big-endian word reads) and 32-bit offsets + lengths. The corpus conditions are
asserted by fz.corpora() and again on a batch that is a subsample. No record
is edited to point outside its frame: tests/test_gpu_dns.py, test_gpu_decap.py,
test_gpu_select.py and test_gpu_flow.py keep the hostile-record cases.

No sweep disagreed with its reference when this suite was written."""
import numpy as np
import pytest

from nex_amd import abi
from nex_amd.engine import FrameBatch
from nex_amd.flow import FlowOption
from nex_amd.frame import ParseMode, ParseOption
from tests import dns_frames as df
from tests import helpers
from tests import second_pass_fuzz as fz
from tests import second_pass_ref as ref
from tests import tunnel_frames as tf
from tests.helpers import packed_from_byte_1, to_host
from tests.test_gpu_decap import outer_offsets
from tests.test_gpu_flow import dummy_batch, flows_from_hashes
from tests.test_gpu_select import check_select

pytestmark = pytest.mark.gpu

VLAN = ParseOption(unwrap_vlan=True)
FROM_IP = ParseOption(from_ip_packet=True, offset=0)


@pytest.fixture(scope="module")
def corp(oracle):
    return fz.corpora(oracle)


def two_layouts(frames):
    """The first and the last layout of tests.helpers.layouts()."""
    return [("packed pad 1 from byte 1", packed_from_byte_1(frames)),
            ("offsets32 + lengths", FrameBatch.from_frames(frames, pad_to=4).with_offsets32())]


def shuffled(frames, recs, seed):
    idx = fz.batch_indices(len(frames), seed)
    return idx, [frames[i] for i in idx], recs[idx]


def per_unique(idx, fn):
    """fn(i) for every batch entry, computed once per corpus index."""
    memo = {i: fn(i) for i in set(idx.tolist())}
    return [memo[i] for i in idx.tolist()]


def test_dns_sweep(engine, corp):
    import torch
    idx, frames, recs = shuffled(corp.dns, corp.dns_recs, fz.SEED + 10)
    if len(set(idx.tolist())) < len(corp.dns):
        fz.check_dns(frames, recs)
    exp = per_unique(idx, lambda i: ref.dns_frame_rows(corp.dns[i], corp.dns_recs[i]))
    n = len(frames)
    want = df.summary_array([s for s, _ in exp])
    k = np.array([len(rows) for _, rows in exp], np.int64)
    before = np.concatenate([[0], np.cumsum(k)])
    tiles = (n + 255) // 256
    tf_want = np.array([before[256 * t] for t in range(tiles)] + [before[n]], np.uint64)
    want["first"] = before[:n] - tf_want[np.arange(n) >> 8].astype(np.int64)
    rows_want = df.entry_array([e for _, rows in exp for e in rows])
    assert len(rows_want) > 3000 and (k > 3).sum() > 100 and (k == 0).sum() > 1000
    for lname, batch in two_layouts(frames):
        drecs = engine.parse(batch, VLAN, out_kind=abi.OUT_RECORD)
        dns, tile_first, entries, total = engine.dns(batch, drecs)
        torch.cuda.synchronize()
        helpers.records_equal(to_host(drecs, abi.RECORD_DTYPE, n), recs, frames, f"{lname}: records")
        helpers.records_equal(to_host(dns, abi.DNS_DTYPE, n), want, frames, f"{lname}: summaries")
        assert (tile_first.cpu().numpy().astype(np.uint64) == tf_want).all(), lname
        assert total == len(rows_want), (lname, total, len(rows_want))
        helpers.records_equal(to_host(entries, abi.DNS_ENTRY_DTYPE, total), rows_want, None, f"{lname}: entries")
    cap = len(rows_want) // 2  # a capacity below the total: the rows below it are the same
    _, tf2, e2, t2 = engine.dns(batch, drecs, entries_cap=cap)
    torch.cuda.synchronize()
    assert int(t2.item()) == len(rows_want) and e2.numel() == cap * 16
    helpers.records_equal(to_host(e2, abi.DNS_ENTRY_DTYPE, cap), rows_want[:cap], None, "entries below the capacity")


def test_decap_sweep(engine, corp, oracle):
    import torch
    idx, frames, recs = shuffled(corp.tun, corp.tun_recs, fz.SEED + 11)
    if len(set(idx.tolist())) < len(corp.tun):
        fz.check_decap(frames, recs)
    n = len(frames)
    for li, (lname, batch) in enumerate(two_layouts(frames)):
        drecs = engine.parse(batch, VLAN, out_kind=abi.OUT_RECORD)
        torch.cuda.synchronize()
        helpers.records_equal(to_host(drecs, abi.RECORD_DTYPE, n), recs, frames, f"{lname}: records")
        off = outer_offsets(batch)
        for port in (abi.VXLAN_PORT, fz.CUSTOM_VXLAN_PORT)[: 2 - li]:
            name = f"{lname} port {port}"
            exp = per_unique(idx, lambda i: ref.decap_frame(corp.tun[i], corp.tun_recs[i], vxlan_port=port))
            tunnels, inner = engine.decap(batch, drecs, vxlan_port=port)
            torch.cuda.synchronize()
            htun = to_host(tunnels, abi.TUNNEL_DTYPE, n)
            ioff, ilen = to_host(inner.offsets, np.int64, n), to_host(inner.lengths, np.uint32, n)
            helpers.records_equal(htun, tf.tunnels_array([t for t, _, _ in exp]), frames, f"{name}: tunnels")
            assert (ioff - off == np.array([o for _, o, _ in exp], np.int64)).all(), name
            assert (ilen == np.array([ln for _, _, ln in exp], np.uint32)).all(), name
            # decap_select + parse of each inner class == the oracle's parse of the inner bytes cut out on the host
            for classes, option, flags in (({abi.INNER_ETHERNET}, ParseOption(), 0),
                                           ({abi.INNER_IPV4, abi.INNER_IPV6}, FROM_IP, abi.PARSE_FROM_IP)):
                pick = [i for i, (t, _, _) in enumerate(exp)
                        if t["kind"] != abi.TUN_NONE and t["status"] == abi.FRAME_OK and t["inner"] in classes]
                cut = [frames[i][exp[i][1]: exp[i][1] + exp[i][2]] for i in pick]
                assert len(pick) > 100, (name, classes)
                sidx, sel = engine.decap_select(tunnels, inner, classes)
                assert sel.count == len(pick), (name, classes)
                assert (to_host(sidx, np.uint32, sel.count) == np.array(pick)).all(), (name, classes)
                assert (to_host(sel.offsets, np.int64, sel.count) == ioff[pick]).all(), (name, classes)
                assert (to_host(sel.lengths, np.uint32, sel.count) == ilen[pick]).all(), (name, classes)
                got = engine.parse_to_numpy(sel, option, out_kind=abi.OUT_RECORD)
                helpers.records_equal(got, fz.oracle_records(oracle, cut, flags), cut, f"{name}: inner parse {classes}")


def test_select_sweep(engine, corp):
    import torch
    idx, frames, recs = shuffled(corp.sel, corp.sel_recs, fz.SEED + 12)
    picks = corp.gpu_filters()
    for lname, batch in two_layouts(frames):
        drecs = engine.parse(batch, VLAN, ParseMode.Strict, out_kind=abi.OUT_RECORD)
        torch.cuda.synchronize()
        helpers.records_equal(to_host(drecs, abi.RECORD_DTYPE, len(frames)), recs, frames, f"{lname}: records")
        for k in picks:
            sel, rule = corp.verdicts(k)
            check_select(engine, f"{lname} filter {k}: {corp.filters[k]}", batch, drecs, corp.filters[k], sel[idx], rule[idx])


def test_flow_sweep(engine, corp):
    import torch
    idx, frames, recs = shuffled(corp.flow, corp.flow_recs, fz.SEED + 13)
    lengths = [len(f) for f in corp.flow]
    for li, (lname, batch) in enumerate(two_layouts(frames)):
        drecs = engine.parse(batch, VLAN, ParseMode.Strict, out_kind=abi.OUT_RECORD)
        torch.cuda.synchronize()
        helpers.records_equal(to_host(drecs, abi.RECORD_DTYPE, len(frames)), recs, frames, f"{lname}: records")
        for kname, key in (corp.keys if li == 0 else corp.keys[:1]):
            for sym, ports in ((False, True), (True, True), (False, False), (True, False)):
                want = ref.flow_rows(corp.flow, corp.flow_recs, lengths, sym, ports, key)[idx]
                got = to_host(engine.flow(batch, drecs, FlowOption(symmetric=sym, ports=ports, key=key)), abi.FLOW_DTYPE,
                              batch.count)
                bad = np.nonzero(got != want)[0]
                assert len(bad) == 0, (lname, kname, sym, ports, len(bad), int(bad[0]), got[bad[0]], want[bad[0]],
                                       frames[bad[0]].hex())


@pytest.mark.parametrize("count", [1025, 4097])
def test_partition_sweep(engine, count):
    batch = dummy_batch(count)
    for buckets in fz.BUCKETS:
        for hname, hashes in fz.partition_hashes(count, buckets).items():
            name = f"n={count} buckets={buckets} {hname}"
            want_idx, want_first = ref.partition(hashes, buckets)
            idx, table, first = engine.flow_partition(batch, flows_from_hashes(hashes), buckets)
            assert first.tolist() == want_first.tolist(), name
            got = to_host(idx, np.uint32, count)
            bad = np.nonzero(got != want_idx)[0]
            assert len(bad) == 0, (name, int(bad[0]), int(got[bad[0]]), int(want_idx[bad[0]]))
            assert (to_host(table.offsets, np.int64, count) == want_idx.astype(np.int64) * 4).all(), name
            assert (to_host(table.lengths, np.uint32, count) == 4).all(), name
