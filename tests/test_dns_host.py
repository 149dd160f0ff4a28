"""CPU: the host side of the DNS message pass. nex_amd.dns (dns_host,
decode_dns_name, the DnsPacket view, the mnemonic tables) reproduces the byte
vectors the reference's own unit tests assert (tests/golden/dns_vectors.json:
dns.rs:1400-1519), the generator of the GPU tests agrees with dns_host,
include/nexg.h and nex_amd/abi.py agree on the new structs, and
nex_amd.dns_dump prints the lines of dns_dump.rs:102-147."""
import ctypes
import ipaddress
import os
import re
import subprocess

import pytest

from nex_amd import abi, dns, dns_dump
from oracle import oracle
from tests import dns_frames as df

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "nexg.h")
LIB = os.path.join(ROOT, "nex_amd", "libnexg.so")


def _packet(raw):
    s, entries = dns.dns_host(raw)
    s["msg_off"] = 0
    return s, entries, dns.DnsPacket(raw, s, entries)


def test_reference_query_and_response_vectors():
    """dns.rs:1400-1434: a lone query and a lone resource record, walked as
    the first query / answer of a message."""
    g = df.vectors()
    for v in g["query"]:
        raw = bytes.fromhex(v["bytes"])
        s, entries, p = _packet(df.header(1, 0, 1) + raw)
        assert (s["status"], s["n_q"], s["rest_off"]) == (abi.FRAME_OK, 1, 12 + len(raw)), v["name"]
        q = p.queries[0]
        assert q.qname.hex() == v["fields"]["qname"] and entries[0]["name"] == len(q.qname)
        assert repr(q.qtype) == v["fields"]["qtype"] and repr(q.qclass) == v["fields"]["qclass"]
    for v in g["response"]:
        raw = bytes.fromhex(v["bytes"])
        s, entries, p = _packet(df.header(1, 0x8000, 0, 1) + raw)
        assert (s["status"], s["n_an"], s["flags8"], s["rest_off"]) == (abi.FRAME_OK, 1, 1, 12 + len(raw)), v["name"]
        r, f = p.responses[0], v["fields"]
        assert (repr(r.rtype), repr(r.rclass), r.ttl, r.data_len, list(r.data)) == \
            (f["rtype"], f["rclass"], f["ttl"], f["data_len"], f["data"])
        assert r.name_tag == 0xC00C and entries[0]["flags8"] == 0


def test_reference_packet_vectors():
    """dns.rs:1437-1481."""
    for v in df.vectors()["packet"]:
        raw = bytes.fromhex(v["bytes"])
        s, entries, p = _packet(raw)
        assert s["status"] == abi.FRAME_OK and s["rest_off"] == len(raw) and p.payload == b"", v["name"]
        h = v["header"]
        assert (p.id, p.is_response, p.query_count) == (h["id"], h["is_response"], h["query_count"])
        assert p.response_count == h.get("response_count", 0) == s["an"]
        assert len(p.queries) == len(v["queries"]) == s["n_q"] and len(p.responses) == len(v["responses"]) == s["n_an"]
        for q, w in zip(p.queries, v["queries"]):
            assert q.qname_parsed() == w["qname_parsed"] and repr(q.qtype) == w["qtype"]
            assert repr(q.qclass) == w.get("qclass", "IN")
        for r, w in zip(p.responses, v["responses"]):
            assert (repr(r.rtype), repr(r.rclass), r.ttl, r.data_len, list(r.data)) == \
                (w["rtype"], w["rclass"], w["ttl"], w["data_len"], w["data"])
        assert len(entries) == s["n_q"] + s["n_an"] and [e["section"] for e in entries] == sorted(e["section"] for e in entries)


def test_reference_name_vectors():
    """dns.rs:1499-1519: the loop vector and the compressed qname."""
    for v in df.vectors()["name"]:
        raw = bytes.fromhex(v["bytes"])
        if "error" in v:
            with pytest.raises(dns.DnsNameError) as e:
                dns.decode_dns_name(raw, 0)
            assert e.value.kind == v["error"], v["name"]
        else:
            assert dns.decode_dns_name(raw, 0) == (v["parsed"], 6), v["name"]  # 03 www + the pointer's 2 bytes
            q = dns.DnsQuery(raw + b"\x00\x01\x00\x01", dict(off=0, name=len(raw), type=1, dns_class=1))
            assert q.qname_parsed() == v["parsed"] and q.qname == raw


def test_decode_dns_name_rules():
    """dns.rs:1303-1390: every error kind, the consumed count, depth 16."""
    d = dns.decode_dns_name

    def kind(buf, start=0):
        with pytest.raises(dns.DnsNameError) as e:
            d(bytes(buf), start)
        return e.value.kind, e.value.context

    assert d(b"\x00") == ("", 1)
    assert d(b"\x03abc\x02de\x00") == ("abc.de", 8)
    assert d(b"\xff\x03abc\x00", 1) == ("abc", 5)
    assert kind(b"") == ("Truncated", "DNS name")
    assert kind(b"\x03abc") == ("Truncated", "DNS name")          # no terminator
    assert kind(b"\x05abc") == ("Truncated", "DNS label")
    assert kind(b"\x01a\xc0") == ("Truncated", "DNS compression pointer")
    assert kind(b"\xc0\x02") == ("InvalidCompression", "DNS compression pointer")  # target == len
    assert kind(b"\x40a\x00") == ("InvalidCompression", "DNS label encoding")
    assert kind(b"\x80a\x00") == ("InvalidCompression", "DNS label encoding")
    assert kind(b"\x02\xff\xfe\x00") == ("InvalidUtf8", "DNS label")
    assert kind(b"\xc0\x00") == ("CompressionLoop", "DNS name")
    assert d(b"\x01a\x00\x01b\xc0\x00", 3) == ("b.a", 4)           # consumed stops at the pointer
    # a chain of 16 pointers decodes, 17 do not (each points at the next; distinct targets)
    for jumps, ok in ((16, True), (17, False)):
        buf = bytearray()
        for j in range(jumps):
            buf += bytes([0xC0, 2 * (j + 1)])
        buf += b"\x01z\x00"
        if ok:
            assert d(bytes(buf)) == ("z", 2)
        else:
            assert kind(buf) == ("CompressionLoop", "DNS name")


def test_mnemonic_tables():
    assert [repr(dns.DnsType(v)) for v in (1, 28, 33, 53, 54, 65, 66, 99, 109, 110, 249, 260, 261, 32768, 32769, 0)] == \
        ["A", "AAAA", "SRV", "SMIMEA", "Unknown(54)", "HTTPS", "Unknown(66)", "SPF", "EUI64", "Unknown(110)", "TKEY",
         "AMTRELAY", "Unknown(261)", "TA", "DLV", "Unknown(0)"]
    assert repr(dns.DnsType(23)) == "NSAP_PTR" and repr(dns.DnsType(41)) == "OPT" and repr(dns.DnsType(255)) == "ANY"
    assert [repr(dns.DnsClass(v)) for v in (1, 2, 3, 4, 5, 255)] == ["IN", "CS", "CH", "HS", "Unknown(5)", "Unknown(255)"]
    assert [repr(dns.OpCode(v)) for v in (0, 1, 2, 4, 5, 6, 7)] == \
        ["Query", "InverseQuery", "Status", "Notify", "Update", "Dso", "Unassigned(7)"]
    assert [repr(dns.RetCode(v)) for v in (0, 2, 3, 5, 11, 15)] == \
        ["NoError", "ServFail", "NXDomain", "Refused", "Dsotypeni", "BadMode"]
    assert repr(dns.RetCode(20)) == "Unassigned(20)"
    assert len(dns.DnsType.TABLE) == 53 + 11 + 11 + 12 + 2


def test_generator_agrees_with_dns_host():
    """Each generated case's implied status, counts, entries and names are
    what dns_host finds; under the oracle's record the candidate rules give
    the case's own expectation for the default port, any_udp and port 5353,
    with and without the VLAN extension."""
    cases = df.cases()
    df.check_cases_against_host(cases)
    assert {c.status for c in cases if c.msg is not None} == {abi.FRAME_OK, abi.ERR_BUFFER_TOO_SHORT, abi.ERR_MALFORMED}
    for c in cases:
        for vlan_parsed in (True, False):
            rec = oracle.parse_frame(c.frame, abi.PARSE_VLAN if vlan_parsed else 0)
            for port, any_udp in ((53, False), (0, False), (53, True), (5353, False)):
                got, entries = dns.dns_frame_host(c.frame, rec, port, any_udp)
                want, wentries = c.expect(port, any_udp, vlan_parsed)
                assert got == want and entries == wentries, (c.what, vlan_parsed, port, any_udp, got, want)
    by = {c.what: c for c in cases}
    assert not by["udp to another port"].candidate() and by["udp to another port"].candidate(any_udp=True)
    assert not by["udp to 5353"].candidate() and by["udp to 5353"].candidate(port=5353)
    assert by["vlan-tagged query"].candidate() and not by["vlan-tagged query"].candidate(vlan_parsed=False)
    # a record reaching past its frame, an error status: no candidate
    c = by["reference query packet"]
    rec = oracle.parse_frame(c.frame)
    assert dns.dns_frame_host(c.frame, rec)[0]["flags8"] == 1
    for tamper in (dict(payload_len=int(rec["payload_len"]) + 1), dict(payload_off=int(rec["payload_off"]) + 1),
                   dict(flags=int(rec["flags"]) | abi.ERR_TRUNCATED << abi.STATUS_SHIFT)):
        r = {n: int(rec[n]) for n in ("flags", "payload_off", "payload_len", "src_port", "dst_port")}
        r.update(tamper)
        assert dns.dns_frame_host(c.frame, r) == (dict(dict.fromkeys(dns.SUMMARY_FIELDS, 0), msg_off=0), [])


def test_dns_layouts_match_c(tmp_path):
    names, enames = abi.DNS_DTYPE.names, abi.DNS_ENTRY_DTYPE.names
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HDR}"', 'int main(void){',
             'printf("%zu %zu %zu\\n", sizeof(nexg_dns), sizeof(nexg_dns_entry), sizeof(nexg_dns_option));']
    lines += [f'printf("%zu\\n", offsetof(nexg_dns, {f}));' for f in names]
    lines += [f'printf("%zu\\n", offsetof(nexg_dns_entry, {f}));' for f in enames]
    lines += [f'printf("%zu\\n", offsetof(nexg_dns_option, {f}));' for f, _ in abi.DnsOption._fields_]
    counts = (0, 1, 256, 257, 65536, 65537, 4294967295)
    lines += ['printf("%u\\n", (unsigned)NEXG_DNS_ANY_UDP);']
    lines += [f'printf("%llu\\n", (unsigned long long)nexg_dns_tile_first_bytes({n}ull));' for n in counts]
    lines.append("return 0;}")
    src = tmp_path / "probe_dns.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe_dns"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    out = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    assert out[:3] == [32, 16, 8] == [abi.DNS_DTYPE.itemsize, abi.DNS_ENTRY_DTYPE.itemsize, ctypes.sizeof(abi.DnsOption)]
    o = out[3:]
    assert o[:len(names)] == [abi.DNS_DTYPE.fields[f][1] for f in names]
    o = o[len(names):]
    assert o[:len(enames)] == [abi.DNS_ENTRY_DTYPE.fields[f][1] for f in enames]
    o = o[len(enames):]
    assert o[:3] == [getattr(abi.DnsOption, f).offset for f, _ in abi.DnsOption._fields_]
    assert o[3] == abi.DNS_ANY_UDP
    assert o[4:] == [abi.dns_tile_first_bytes(n) for n in counts] == [8 * ((n + 255) // 256 + 1) for n in counts]


def test_header_declares_and_library_exports():
    text = open(HDR).read()
    for fn in ("nexg_dns_batch", "nexg_dns_entries"):
        assert re.search(r"^int " + fn + r"\(nexg_ctx\* ctx,", text, re.M), fn
        assert fn in abi.EXPORTED_SYMBOLS
    assert "nexg_dns_tile_first_bytes" in abi.HEADER_INLINE
    assert os.path.exists(LIB), "libnexg.so not built"
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {"nexg_dns_batch", "nexg_dns_entries"} <= exported
    from nex_amd import _lib
    lib = _lib.load()
    assert lib.nexg_dns_batch.argtypes is not None and lib.nexg_dns_entries.argtypes is not None


def _lines(msg, src="10.1.2.3", sport=53, dst="10.4.5.6", dport=49153):
    s, entries = dns.dns_host(msg)
    s["msg_off"] = 0
    return dns_dump.dns_lines(ipaddress.ip_address(src), sport, ipaddress.ip_address(dst), dport,
                              dns.DnsPacket(msg, s, entries))


def test_dns_dump_lines():
    """dns_dump.rs:102-147 on hand-written expected lines."""
    g = df.vectors()["packet"]
    assert _lines(bytes.fromhex(g[0]["bytes"]), "192.168.122.1", 49153, "192.168.122.189", 53) == [
        "DNS Packet: 192.168.122.1:49153 > 192.168.122.189:53",
        '  Query: Ok("_ldap._tcp.dc._msdcs.S4DOM.PRIVATE") (type: SRV, class: IN)']
    assert _lines(bytes.fromhex(g[1]["bytes"]), "fe80::1", 53, "2001:db8::2", 49153) == [
        "DNS Packet: fe80::1:53 > 2001:db8::2:49153",
        '  Query: Ok("s4dc1.samba.windows8.private") (type: A, class: IN)',
        "  Response: 192.168.122.189 (type: A, ttl: 900)"]
    m = (df.Message(7, 0x8180).query("host.example", 255, 3).query("odd", 65280, 7)
         .record(1, 28, bytes.fromhex("20010db8000000000000000000000001"), ttl=60)
         .record(1, 5, df.qname("alias.example.net"), ttl=61)
         .record(1, 16, b"\x05hello\x0csecond \"one\"", ttl=62)
         .record(1, 65280, b"\x01\x02", ttl=63)
         .record(1, 12, b"\x03ptr\xc0\x00", ttl=64)   # a pointer loop inside the record's own data
         .record(1, 12, b"\x03ptr\x02ok\x00", ttl=68)
         .record(1, 1, b"\x01\x02\x03", ttl=65)
         .record(1, 2, b"\x05ab", ttl=66)
         .record(1, 16, b"\x02\xff\xfe", ttl=67)
         .record(2, 1, bytes(4)))
    assert _lines(m.bytes()) == [
        "DNS Packet: 10.1.2.3:53 > 10.4.5.6:49153",
        '  Query: Ok("host.example") (type: ANY, class: CH)',
        '  Query: Ok("odd") (type: Unknown(65280), class: Unknown(7))',
        "  Response: 2001:db8::1 (type: AAAA, ttl: 60)",
        "  Response: alias.example.net (type: CNAME, ttl: 61)",
        '  TXT: "hello" (ttl: 62)',
        '  TXT: "second "one"" (ttl: 62)',
        "  Invalid name data for type: PTR",
        "  Response: ptr.ok (type: PTR, ttl: 68)",
        "  Invalid IP data for type: A",
        "  Invalid name data for type: NS",
        "  Invalid TXT data"]
    # a qname that does not decode prints the error's variant name
    bad = df.Message(8, 0x0100).query(None, 1, 1, raw=b"\x02\xc0\x00\x00")
    assert _lines(bad.bytes())[1] == "  Query: Err(InvalidUtf8) (type: A, class: IN)"
    loop = df.Message(9, 0x0100).query(None, 1, 1, raw=b"\x01\x00\x00")  # label "\0", then the end
    assert _lines(loop.bytes())[1] == '  Query: Ok("\\0") (type: A, class: IN)'
