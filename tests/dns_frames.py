"""DNS test traffic: hand-built DNS messages wrapped in Eth/IPv4/UDP and
Eth/IPv6/UDP, with the edge and negative cases of nexg_dns_batch
(include/nexg.h). Every case carries what its construction implies (status,
counts, entry list, names), so the expectation does not come from the code
under test; check_cases_against_host() cross-checks the list against
nex_amd.dns.dns_host."""
import json
import os
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from nex_amd import abi
from nex_amd import dns as hostdns
from tests import helpers
from tests.helpers import _eth, _ipv4, _ipv6, _tcp

VECTORS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dns_vectors.json")
OK, SHORT, BAD = abi.FRAME_OK, abi.ERR_BUFFER_TOO_SHORT, abi.ERR_MALFORMED
CLIENT = 0xC001  # the other port of every wrapped message


def vectors():
    with open(VECTORS) as f:
        return json.load(f)


@dataclass
class Case:
    frame: bytes
    msg: Optional[bytes]     # the UDP payload (None: the frame carries no parsed, non-empty UDP payload)
    msg_off: int = 0
    sport: int = 0
    dport: int = 0
    status: int = OK         # of the message, wherever it is a candidate
    flags8: int = 0
    counts: tuple = (0, 0, 0, 0)  # n_q, n_an, n_ns, n_ar
    rest_off: int = 0
    entries: List[dict] = field(default_factory=list)
    names: List[Optional[str]] = field(default_factory=list)  # per query: the decoded name, or an error kind "!Kind"
    vlan: bool = False       # a UDP frame only when parsed with NEXG_PARSE_VLAN
    what: str = ""

    def candidate(self, port=53, any_udp=False, vlan_parsed=True):
        if self.msg is None or (self.vlan and not vlan_parsed):
            return False
        return any_udp or (port or 53) in (self.sport, self.dport)

    def expect(self, port=53, any_udp=False, vlan_parsed=True):
        """(summary fields but `first`, entries) nexg_dns_batch must report."""
        s = dict.fromkeys(hostdns.SUMMARY_FIELDS, 0)
        s["msg_off"] = 0
        if not self.candidate(port, any_udp, vlan_parsed):
            return s, []
        s["status"] = self.status
        if self.status == SHORT:
            return s, []
        m = self.msg
        be = lambda p: int.from_bytes(m[p:p + 2], "big")
        s.update(flags8=self.flags8, msg_off=self.msg_off, msg_len=len(m), id=be(0), flags=be(2), qd=be(4), an=be(6),
                 ns=be(8), ar=be(10))
        if self.status == BAD:
            return s, []
        s.update(n_q=self.counts[0], n_an=self.counts[1], n_ns=self.counts[2], n_ar=self.counts[3],
                 rest_off=self.rest_off)
        return s, self.entries


def udp(payload: bytes, sport: int, dport: int) -> bytes:
    ln = 8 + len(payload)
    return sport.to_bytes(2, "big") + dport.to_bytes(2, "big") + ln.to_bytes(2, "big") + b"\x00\x00" + payload


def wrap(payload: bytes, sport: int, dport: int, v6: bool) -> bytes:
    u = udp(payload, sport, dport)
    return _eth(_ipv6(u, 17), 0x86DD) if v6 else _eth(_ipv4(u, 17))


def header(ident, flags, qd=0, an=0, ns=0, ar=0) -> bytes:
    return b"".join(v.to_bytes(2, "big") for v in (ident, flags, qd, an, ns, ar))


def qname(name: str) -> bytes:
    if not name:
        return b"\x00"
    return b"".join(bytes([len(l)]) + l.encode() for l in name.split(".")) + b"\x00"


class Message:
    """A DNS message built piece by piece; each piece records the entry its
    position and fields imply."""

    def __init__(self, ident, flags, qd=None, an=None, ns=None, ar=None):
        self.declared = [qd, an, ns, ar]
        self.ident, self.flags = ident, flags
        self.body = b""
        self.entries, self.names = [], []
        self.counts = [0, 0, 0, 0]

    def query(self, name, qtype=1, qclass=1, raw=None, decoded=None):
        qn = qname(name) if raw is None else raw
        self.entries.append(dict(section=0, flags8=0, off=12 + len(self.body), type=qtype, dns_class=qclass, ttl=0,
                                 name=len(qn), data_len=0))
        self.names.append(name if decoded is None else decoded)
        self.body += qn + qtype.to_bytes(2, "big") + qclass.to_bytes(2, "big")
        self.counts[0] += 1
        return self

    def record(self, section, rtype, data, name_tag=0xC00C, rclass=1, ttl=300, data_len=None, present=None):
        """`data_len` declared (default: the data's length); `present` bytes of
        the data actually in the message (default: all)."""
        dl = len(data) if data_len is None else data_len
        data = data if present is None else data[:present]
        self.entries.append(dict(section=section, flags8=1 if dl > len(data) else 0, off=12 + len(self.body), type=rtype,
                                 dns_class=rclass, ttl=ttl, name=name_tag, data_len=dl))
        self.body += (name_tag.to_bytes(2, "big") + rtype.to_bytes(2, "big") + rclass.to_bytes(2, "big") +
                      ttl.to_bytes(4, "big") + dl.to_bytes(2, "big") + data)
        self.counts[section] += 1
        return self

    def bytes(self, tail=b""):
        d = [c if x is None else x for c, x in zip(self.counts, self.declared)]
        return header(self.ident, self.flags, *d) + self.body + tail


def make(what, m: Message, sport=CLIENT, dport=53, v6=False, tail=b"", **kw):
    """A Case from a built message. `tail`: bytes after the last record, too
    few for another one (the DnsPacket payload: rest_off = n - len(tail))."""
    msg = m.bytes(tail)
    d = [c if x is None else x for c, x in zip(m.counts, m.declared)]
    short = any(c < x for c, x in zip(m.counts[1:], d[1:]))
    frame = wrap(msg, sport, dport, v6)
    return Case(frame, msg, msg_off=len(frame) - len(msg), sport=sport, dport=dport, status=OK,
                flags8=abi.DNS_CANDIDATE | (abi.DNS_SECTION_SHORT if short else 0), counts=tuple(m.counts),
                rest_off=len(msg) - len(tail), entries=m.entries, names=m.names, what=what, **kw)


def raw_case(what, msg, status, sport=CLIENT, dport=53, v6=False):
    """A message whose walk fails (or is too short): no counts, no entries."""
    frame = wrap(msg, sport, dport, v6)
    return Case(frame, msg, msg_off=len(frame) - len(msg), sport=sport, dport=dport, status=status,
                flags8=abi.DNS_CANDIDATE if status == BAD else 0, what=what)


A4 = bytes([192, 0, 2, 7])
A6 = bytes(range(0x20, 0x30))


def cases():
    g = vectors()
    out = []
    # the reference's two packet vectors: a query to port 53, a response from it
    v = g["packet"][0]
    raw = bytes.fromhex(v["bytes"])
    m = Message(0x9BA0, 0x0100).query("_ldap._tcp.dc._msdcs.S4DOM.PRIVATE", 33, 1)
    assert m.bytes() == raw
    out.append(make("reference query packet", m))
    v = g["packet"][1]
    raw = bytes.fromhex(v["bytes"])
    m = Message(0xBC12, 0x8580).query("s4dc1.samba.windows8.private", 1, 1).record(1, 1, bytes([192, 168, 122, 189]),
                                                                                   ttl=900)
    assert m.bytes() == raw
    out.append(make("reference response packet", m, sport=53, dport=CLIENT, v6=True))
    # short payloads
    out.append(raw_case("payload 1 B", b"\x9b", SHORT))
    out.append(raw_case("payload 11 B", header(1, 0x0100, 1)[:11], SHORT, v6=True))
    out.append(make("12 B, all counts 0", Message(0x1111, 0x0100)))
    out.append(raw_case("12 B, qd = 1", header(0x1112, 0x0100, 1), BAD))
    out.append(make("root-name query", Message(0x1113, 0x0100).query("", 2, 1), v6=True))
    out.append(raw_case("label past the end", header(0x1114, 0x0100, 1) + b"\x05ab", BAD))
    out.append(raw_case("qname 0xC0 0x0C is a length of 192, bytes missing",
                        header(0x1115, 0x0100, 1) + b"\xc0\x0c\x00\x01\x00\x01", BAD, v6=True))
    # the same with the 192 bytes there: one 192-B label to the walk; the name decoder, over the qname alone,
    # follows C0 0C to qname byte 12
    label = b"\x0c" + b"x" * 10 + b"\x03abc\x00" + b"y" * (192 - 16)
    assert len(label) == 192
    out.append(make("qname 0xC0 + 192 bytes present",
                    Message(0x1116, 0x0100).query(None, 1, 1, raw=b"\xc0" + label + b"\x00", decoded="abc")))
    out.append(raw_case("type and class cut to 3 B", header(0x1117, 0x0100, 1) + qname("a") + b"\x00\x01\x00", BAD))
    out.append(make("qd = 2", Message(0x1118, 0x0100).query("one.example", 1, 1).query("two.example.org", 28, 1),
                    v6=True))
    out.append(make("qd = 0 with answers", Message(0x1119, 0x8180).record(1, 1, A4).record(1, 28, A6, ttl=7),
                    sport=53, dport=CLIENT))
    out.append(make("data_len beyond the end",
                    Message(0x111A, 0x8180).query("cut.example").record(1, 16, bytes(100), present=5),
                    sport=53, dport=CLIENT, v6=True))
    out.append(make("11 B left before a declared record",
                    Message(0x111B, 0x8180, an=2, ns=1).query("short.example").record(1, 1, A4),
                    sport=53, dport=CLIENT, tail=bytes(range(11))))
    out.append(make("an = 65535 with two real records",
                    Message(0x111C, 0x8180, an=65535).query("many.example").record(1, 1, A4).record(1, 1, A4, ttl=1),
                    sport=53, dport=CLIENT, v6=True))
    out.append(make("records in all three sections",
                    Message(0x111D, 0x8580).query("all.example", 255, 1).record(1, 5, qname("cname.example"))
                    .record(2, 2, qname("ns.example"), ttl=86400).record(3, 41, b"", name_tag=0x0000, rclass=1232, ttl=0),
                    sport=53, dport=CLIENT))
    out.append(make("trailing bytes after the last record",
                    Message(0x111E, 0x8180).query("tail.example").record(1, 1, A4), sport=53, dport=CLIENT, v6=True,
                    tail=bytes(range(40))))
    # an uncompressed owner name is read as name_tag / type / class / ttl / data_len all the same
    own = qname("www.example.com") + b"\x00\x01\x00\x01\x00\x00\x00\x3c\x00\x04" + A4
    be = lambda p, n=2: int.from_bytes(own[p:p + n], "big")
    m = Message(0x111F, 0x8180, an=1)
    m.entries.append(dict(section=1, flags8=1, off=12, type=be(2), dns_class=be(4), ttl=be(6, 4), name=be(0),
                          data_len=be(10)))
    m.counts[1] = 1
    m.body = own
    assert be(10) > len(own) - 12
    out.append(make("record with an uncompressed name", m, sport=53, dport=CLIENT))
    out.append(make("txt and unknown type", Message(0x1120, 0x8180).query("txt.example", 16, 3)
                    .record(1, 16, b"\x05hello\x05world").record(1, 65280, b"\x01\x02\x03", rclass=254),
                    sport=53, dport=CLIENT, v6=True))
    # non-candidates
    q = Message(0x2221, 0x0100).query("other.example")
    out.append(make("udp to another port", q, dport=5300))
    out.append(make("udp to 5353", Message(0x2222, 0x0000).query("_http._tcp.local", 12, 1), sport=5353, dport=5353,
                    v6=True))
    out.append(Case(_eth(_ipv4(_tcp(q.bytes()), 6)), None, what="tcp port 0x50"))
    tcp53 = bytearray(_tcp(q.bytes()))
    tcp53[2:4] = (53).to_bytes(2, "big")
    out.append(Case(_eth(_ipv4(bytes(tcp53), 6)), None, what="tcp port 53"))
    out.append(Case(wrap(q.bytes(), CLIENT, 53, False)[:30], None, what="error status: cut inside the IPv4 header"))
    out.append(Case(wrap(b"", CLIENT, 53, True), None, what="udp with an empty payload"))
    out.append(Case(b"", None, what="empty frame"))
    c = make("vlan-tagged query", Message(0x2223, 0x0100).query("vlan.example", 28, 1), vlan=True)
    c.frame = helpers.vlan(c.frame, [0x0064])
    c.msg_off += 4
    out.append(c)
    return out


def check_cases_against_host(case_list=None):
    """The case list's own expectation equals dns_host on every message, and
    each query's name decodes to the generator's name."""
    for c in case_list or cases():
        if c.msg is None:
            continue
        s, entries = hostdns.dns_host(c.msg)
        want, wentries = c.expect(any_udp=True)
        for k in hostdns.SUMMARY_FIELDS:
            assert s[k] == want[k], (c.what, k, s[k], want[k])
        assert entries == wentries, (c.what, entries, wentries)
        assert decoded_names(c.msg, entries) == c.names, c.what


def decoded_names(msg, entries):
    """The decoded qname of every query entry (or "!<error kind>")."""
    out = []
    for e in entries:
        if int(e["section"]) != 0:
            continue
        try:
            out.append(hostdns.decode_dns_name(msg[int(e["off"]):int(e["off"]) + int(e["name"])], 0)[0])
        except hostdns.DnsNameError as err:
            out.append("!" + err.kind)
    return out


def cycled(case_list, count):
    return [case_list[i % len(case_list)] for i in range(count)]


def summary_array(summaries):
    """abi.DNS_DTYPE array from expect()'s dicts (`first` left 0)."""
    a = np.zeros(len(summaries), abi.DNS_DTYPE)
    for i, s in enumerate(summaries):
        for n in abi.DNS_DTYPE.names:
            if n != "first":
                a[i][n] = s[n]
    return a


def entry_array(entries):
    a = np.zeros(len(entries), abi.DNS_ENTRY_DTYPE)
    for i, e in enumerate(entries):
        for n in abi.DNS_ENTRY_DTYPE.names:
            a[i][n] = e[n]
    return a
