"""CPU: the host contracts of the four second passes (nex_amd.dns, tunnel,
select, flow) equal the independent references of tests/second_pass_ref.py on
the whole fuzz corpus of tests/second_pass_fuzz.py, exactly.

Every GPU test of these passes asserts device == contract, so this pins what
they lean on: the contract and the reference were written from different
readings (cursor arithmetic against slice consumption, bit arithmetic against
ipaddress networks, a windowed key against a shift register), and the
references are pinned here by the reference implementation's own asserted
vectors (tests/golden/dns_vectors.json, tunnel_vectors.json) and by the
published RSS vectors (flow_vectors.json). The oracle's records are the input.

No disagreement between a contract and its reference was found when this
suite was written; a frame that shows one belongs in the matching hand corpus
(dns_frames.py, tunnel_frames.py, ...) under a name that says what it is."""
import numpy as np
import pytest

from nex_amd import abi
from nex_amd import dns as hostdns
from nex_amd import flow as hostflow
from nex_amd import select as hostselect
from nex_amd import tunnel as hosttunnel
from tests import dns_frames as df
from tests import flow_frames as ff
from tests import second_pass_fuzz as fz
from tests import second_pass_ref as ref
from tests import tunnel_frames as tf


@pytest.fixture(scope="module")
def corp(oracle):
    return fz.corpora(oracle)


# ---- the references against the reference implementation's own vectors ------------------------

def test_dns_reference_vectors():
    g = df.vectors()
    for v in g["query"]:
        raw = bytes.fromhex(v["bytes"])
        b = ref.Buf(raw)
        q = ref.dns_query_from_buf(b)
        assert q.qname.hex() == v["fields"]["qname"] and b.remaining() == 0, v["name"]
        assert (repr(hostdns.DnsType(q.qtype)), repr(hostdns.DnsClass(q.qclass))) == (v["fields"]["qtype"],
                                                                                   v["fields"]["qclass"])
    for v in g["response"]:
        r, f = ref.dns_response_from_buf(ref.Buf(bytes.fromhex(v["bytes"]))), v["fields"]
        assert (repr(hostdns.DnsType(r.rtype)), repr(hostdns.DnsClass(r.rclass)), r.ttl, r.data_len, list(r.data),
                r.payload) == (f["rtype"], f["rclass"], f["ttl"], f["data_len"], f["data"], b""), v["name"]
    for v in g["packet"] + g["packet_payload"]:
        raw = bytes.fromhex(v["bytes"])
        p = ref.dns_try_from_buf(raw)
        for k, want in v["header"].items():
            assert getattr(p.header, k) == want, (v["name"], k)
        assert p.payload.hex() == v.get("payload", ""), v["name"]
        assert len(p.queries) == len(v.get("queries", [])) and len(p.responses) == len(v.get("responses", []))
        for q, w in zip(p.queries, v.get("queries", [])):
            assert hostdns.decode_dns_name(q.qname, 0)[0] == w["qname_parsed"], v["name"]
            assert repr(hostdns.DnsType(q.qtype)) == w["qtype"], v["name"]
        for r, w in zip(p.responses, v.get("responses", [])):
            assert (repr(hostdns.DnsType(r.rtype)), repr(hostdns.DnsClass(r.rclass)), r.ttl, r.data_len,
                    list(r.data)) == (w["rtype"], w["rclass"], w["ttl"], w["data_len"], w["data"]), v["name"]
    assert ref.dns_try_from_buf(bytes(11)).kind == "BufferTooShort"
    assert ref.dns_try_from_buf(df.header(1, 0, 1)).context == "DNS query section"


def test_tunnel_reference_vectors():
    g = tf.vectors()
    for v in g["gre"]:
        raw = bytes.fromhex(v["bytes"])
        p = ref.gre_try_from_buf(raw)
        assert (p is not None) == v["parsed"], v["name"]
        if p is not None:
            for k, want in v["fields"].items():
                assert getattr(p, k) == want, (v["name"], k)
            assert p.payload.hex() == v["payload"] and len(raw) - len(p.payload) == v["header_len"], v["name"]
            assert ref.gre_tunnel(raw)["hdr_len"] == v["header_len"]
    for v in g["vxlan"]:
        p = ref.vxlan_try_from_buf(bytes.fromhex(v["bytes"]))
        assert p is not None and p.payload.hex() == v["payload"], v["name"]
        for k, want in v["fields"].items():
            assert getattr(p, k) == want, (v["name"], k)
    for v in g["frozen"]:
        raw = bytes.fromhex(v["bytes"])
        p = ref.gre_try_from_buf(raw) if v["kind"] == "gre" else ref.vxlan_try_from_buf(raw)
        assert p.payload.hex() == v["payload"], v["name"]
        for k, want in v["fields"].items():
            assert getattr(p, k) == want, (v["name"], k)
    assert ref.vxlan_try_from_buf(bytes(7)) is None and ref.gre_try_from_buf(bytes(3)) is None


def test_flow_reference_vectors():
    """The shift-register Toeplitz on the published RSS verification vectors."""
    n = 0
    for x in ff.own_corpus():
        if x.hash_l4 is not None:
            assert ref.toeplitz_shift(x.key, hostflow.DEFAULT_KEY) == x.hash_l4, x.what
            assert ref.toeplitz_shift(x.key_ip, hostflow.DEFAULT_KEY) == x.hash_ip, x.what
            n += 1
    assert n == 16
    assert ref.in_prefix(bytes([10, 1, 2, 3]), bytes([10, 0, 0, 0]) + bytes(12), 8)
    assert not ref.in_prefix(bytes([11, 1, 2, 3]), bytes([10, 0, 0, 0]) + bytes(12), 8)
    assert ref.in_prefix(bytes([11, 1, 2, 3]), bytes([10, 0, 0, 0]) + bytes(12), 7)
    assert ref.in_prefix(bytes(16), b"\xff" * 16, 0) and not ref.in_prefix(bytes(15) + b"\x01", bytes(16), 128)


# ---- the contracts against the references on the fuzz corpus ------------------------------------

def test_dns_contract_equals_reference(corp):
    seen = set()
    for i, (f, r) in enumerate(zip(corp.dns, corp.dns_recs)):
        for kw in (dict(), dict(any_udp=True), dict(port=5353)):
            assert hostdns.dns_frame_host(f, r, **kw) == ref.dns_frame_rows(f, r, **kw), (i, kw, f.hex())
        msg = ref.udp_payload(f, r)
        if msg is not None and msg not in seen:
            seen.add(msg)
            assert hostdns.dns_host(msg) == ref.dns_rows(msg), (i, msg.hex())
    assert len(seen) > 3000


def test_decap_contract_equals_reference(corp):
    payloads = set()
    for i, (f, r) in enumerate(zip(corp.tun, corp.tun_recs)):
        for kw in (dict(), dict(vxlan_port=fz.CUSTOM_VXLAN_PORT), dict(which=abi.DECAP_GRE), dict(which=abi.DECAP_VXLAN)):
            assert hosttunnel.decap_host(f, r, **kw) == ref.decap_frame(f, r, **kw), (i, kw, f.hex())
        poff, plen = int(r["payload_off"]), int(r["payload_len"])
        if poff + plen <= len(f):
            payloads.add(bytes(f[poff:poff + plen]))
    for p in payloads:  # both parsers on every payload, whichever the frame's own tunnel kind
        assert hosttunnel.gre_fields(p) == ref.gre_tunnel(p), p.hex()
        assert hosttunnel.vxlan_fields(p) == ref.vxlan_tunnel(p), p.hex()


def test_select_contract_equals_reference(corp):
    assert len(corp.filters) >= 200
    tests_seen = set()
    for k, flt in enumerate(corp.filters):
        sel, rule = corp.verdicts(k)
        for i, (f, r) in enumerate(zip(corp.sel, corp.sel_recs)):
            assert hostselect.match_host(f, r, len(f), flt) == (bool(sel[i]), int(rule[i])), (k, i, flt, f.hex())
        tests_seen |= {r.tests for r in flt.rules}
    assert len(tests_seen) == 200  # every combination of tests the library accepts
    # rule by rule (match_host stops at the first hit), on the frames a rule was made from and their mutations
    for flt in corp.filters[::7]:
        for r in flt.rules:
            for f, rec in zip(corp.sel[::5], corp.sel_recs[::5]):
                assert hostselect.rule_matches(f, rec, len(f), r) == ref.rule_verdict(f, rec, len(f), r), (r, f.hex())


def test_gpu_sweep_filters_exist(corp):
    assert len(corp.gpu_filters()) == 32


def test_flow_contract_equals_reference(corp):
    lengths = [len(f) for f in corp.flow]
    for name, key in corp.keys:
        for sym, ports in ((False, True), (True, True), (False, False), (True, False)):
            opt = hostflow.FlowOption(symmetric=sym, ports=ports, key=key)
            want = ref.flow_rows(corp.flow, corp.flow_recs, lengths, sym, ports, key)
            got = hostflow.flows_host(corp.flow, corp.flow_recs, lengths, opt)
            bad = np.nonzero(got != want)[0]
            assert len(bad) == 0, (name, sym, ports, int(bad[0]), got[bad[0]], want[bad[0]], corp.flow[bad[0]].hex())
    rng = np.random.default_rng(9)
    for name, key in corp.keys:
        for n in (1, 8, 12, 32, 36):
            data = bytes(rng.integers(0, 256, n, dtype=np.uint8))
            assert hostflow.toeplitz(data, fz.key_bytes(key)) == ref.toeplitz_shift(data, fz.key_bytes(key)), (name, n)
    kinds = set(ref.flow_rows(corp.flow, corp.flow_recs, lengths)["kind"].tolist())
    assert kinds == {abi.FLOW_NONE, abi.FLOW_IPV4, abi.FLOW_IPV4_L4, abi.FLOW_IPV6, abi.FLOW_IPV6_L4}
    assert ref.flow_rows(corp.flow, corp.flow_recs, lengths, symmetric=True)["swapped"].sum() > 20


def test_partition_contract_equals_reference():
    for count in (0, 1, 1025, 4097):
        for buckets in fz.BUCKETS:
            for name, hashes in fz.partition_hashes(count, buckets).items():
                gi, gf = hostflow.partition_host(hashes, buckets)
                wi, wf = ref.partition(hashes, buckets)
                assert gi.tolist() == wi.tolist() and gf.tolist() == wf.tolist(), (count, buckets, name)
                if count:
                    b = hashes.astype(np.int64)[wi] % buckets
                    assert (np.diff(b) >= 0).all() and (np.diff(wi.astype(np.int64))[np.diff(b) == 0] > 0).all()
