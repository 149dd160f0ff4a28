"""Host side of the DNS message pass (include/nexg.h nexg_dns_batch /
nexg_dns_entries).

dns_host restates DnsPacket::try_from_buf (nex-packet/src/dns.rs:1166-1259)
for one UDP payload in plain Python: the expectation the device output is
tested against. decode_dns_name is the reference's name decoder
(dns.rs:1303-1390); names are decoded here, on the host, from the offsets the
device entries carry. DnsPacket is a view over (frame bytes, nexg_dns summary,
nexg_dns_entry rows) with the reference's field names.
"""
import ipaddress
from typing import List, Optional, Tuple

from . import abi

DNS_MAX_COMPRESSION_DEPTH = 16  # dns.rs:1301


class DnsNameError(ValueError):
    """A ParseError of decode_dns_name: `kind` is the variant's name
    (Truncated, InvalidCompression, CompressionLoop, InvalidUtf8), `context`
    its context string."""

    def __init__(self, kind: str, context: str):
        super().__init__(f"{kind} ({context})")
        self.kind = kind
        self.context = context


def decode_dns_name(buf: bytes, start: int = 0) -> Tuple[str, int]:
    """dns.rs:1303-1390: (name, bytes consumed at `start`). Pointers index
    into `buf`; a pointer target seen before, or more than 16 jumps, is a
    CompressionLoop; label types 0x40 / 0x80 are InvalidCompression."""
    buf = bytes(buf)
    labels = []
    pos, consumed, jumped, depth = start, 0, False, 0
    visited = []
    while True:
        if pos >= len(buf):
            raise DnsNameError("Truncated", "DNS name")
        ln = buf[pos]
        if not jumped:
            consumed += 1
        if ln == 0:
            break
        if ln & 0xC0 == 0xC0:
            if pos + 1 >= len(buf):
                raise DnsNameError("Truncated", "DNS compression pointer")
            pointer = (ln & 0x3F) << 8 | buf[pos + 1]
            if pointer >= len(buf):
                raise DnsNameError("InvalidCompression", "DNS compression pointer")
            if pointer in visited:
                raise DnsNameError("CompressionLoop", "DNS name")
            visited.append(pointer)
            depth += 1
            if depth > DNS_MAX_COMPRESSION_DEPTH:
                raise DnsNameError("CompressionLoop", "DNS name")
            if not jumped:
                consumed += 1
            pos = pointer
            jumped = True
            continue
        if ln & 0xC0:
            raise DnsNameError("InvalidCompression", "DNS label encoding")
        pos += 1
        if pos + ln > len(buf):
            raise DnsNameError("Truncated", "DNS label")
        try:
            labels.append(buf[pos:pos + ln].decode("utf-8"))
        except UnicodeDecodeError:
            raise DnsNameError("InvalidUtf8", "DNS label") from None
        if not jumped:
            consumed += ln
        pos += ln
    return ".".join(labels), consumed


# ---- value <-> mnemonic tables -------------------------------------------------
# Resource record TYPEs, CLASSes, OpCodes and RCODEs of the IANA "Domain Name
# System (DNS) Parameters" registry, for the values the reference's new()
# functions know (dns.rs:32-40, 162-255, 465-476, 533-557); every other value
# is Unknown(v) / Unassigned(v). Spelt as the reference's enum variants print
# with {:?}: NSAP-PTR is NSAP_PTR.
_TYPES = {i + 1: n for i, n in enumerate(
    "A NS MD MF CNAME SOA MB MG MR NULL WKS PTR HINFO MINFO MX TXT RP AFSDB X25 ISDN RT NSAP NSAP_PTR SIG KEY PX "
    "GPOS AAAA LOC NXT EID NIMLOC SRV ATMA NAPTR KX CERT A6 DNAME SINK OPT APL DS SSHFP IPSECKEY RRSIG NSEC DNSKEY "
    "DHCID NSEC3 NSEC3PARAM TLSA SMIMEA".split())}
_TYPES.update({55 + i: n for i, n in enumerate(
    "HIP NINFO RKEY TALINK CDS CDNSKEY OPENPGPKEY CSYNC ZONEMD SVCB HTTPS".split())})
_TYPES.update({99 + i: n for i, n in enumerate("SPF UINFO UID GID UNSPEC NID L32 L64 LP EUI48 EUI64".split())})
_TYPES.update({249 + i: n for i, n in enumerate(
    "TKEY TSIG IXFR AXFR MAILB MAILA ANY URI CAA AVC DOA AMTRELAY".split())})
_TYPES.update({32768: "TA", 32769: "DLV"})
_CLASSES = {1: "IN", 2: "CS", 3: "CH", 4: "HS"}
_OPCODES = dict(enumerate("Query InverseQuery Status Reserved Notify Update Dso".split()))
# RCODEs 0..11 as the registry numbers them. The reference numbers the
# extended codes BadVers..BadCookie 12..19 (the registry: 16..23); a 4-bit
# header field reaches 12..15 only, and they print as the reference prints them.
_RETCODES = dict(enumerate(
    "NoError FormErr ServFail NXDomain NotImp Refused YXDomain YXRRSet NXRRSet NotAuth NotZone Dsotypeni BadVers "
    "BadKey BadTime BadMode BadName BadAlg BadTrunc BadCookie".split()))


class _Code:
    """A wire value with the reference's Debug spelling: the mnemonic, or
    Unknown(v) / Unassigned(v)."""
    TABLE: dict = {}
    OTHER = "Unknown"

    def __init__(self, value: int):
        self.value = int(value)

    @property
    def name(self) -> Optional[str]:
        return self.TABLE.get(self.value)

    def __repr__(self):
        return self.TABLE.get(self.value) or f"{self.OTHER}({self.value})"

    def __eq__(self, other):
        if isinstance(other, str):
            return self.name == other
        return self.value == (other.value if isinstance(other, _Code) else other)

    def __hash__(self):
        return hash(self.value)


class DnsType(_Code):
    TABLE = _TYPES


class DnsClass(_Code):
    TABLE = _CLASSES


class OpCode(_Code):
    TABLE, OTHER = _OPCODES, "Unassigned"


class RetCode(_Code):
    TABLE, OTHER = _RETCODES, "Unassigned"


# ---- the walk --------------------------------------------------------------------
SUMMARY_FIELDS = ("status", "flags8", "msg_len", "id", "flags", "qd", "an", "ns", "ar", "n_q", "n_an", "n_ns", "n_ar",
                  "rest_off")


def _be16(m, p):
    return m[p] << 8 | m[p + 1]


def dns_host(payload: bytes):
    """DnsPacket::try_from_buf on one non-empty UDP payload as nexg_dns_batch
    reports it: (summary, entries). summary: the nexg_dns fields the message
    alone decides (SUMMARY_FIELDS; msg_off and first belong to the frame and
    the batch); entries: one dict of the nexg_dns_entry fields per query /
    resource record in message order."""
    m = bytes(payload)
    n = len(m)
    s = dict.fromkeys(SUMMARY_FIELDS, 0)
    if n < 12:  # dns.rs:1167-1173
        s["status"] = abi.ERR_BUFFER_TOO_SHORT
        return s, []
    s.update(flags8=abi.DNS_CANDIDATE, msg_len=n, id=_be16(m, 0), flags=_be16(m, 2), qd=_be16(m, 4), an=_be16(m, 6),
             ns=_be16(m, 8), ar=_be16(m, 10))
    entries = []
    pos = 12
    for _ in range(s["qd"]):  # DnsQueryPacket::from_buf_mut, dns.rs:752-790
        start = pos
        ok = True
        while True:
            if pos >= n:
                ok = False
                break
            ln = m[pos]
            pos += 1
            if ln == 0:
                break
            if n - pos < ln:  # a plain length: 0xC0..0xFF are no pointers here
                ok = False
                break
            pos += ln
        if not ok or n - pos < 4:  # dns.rs:1228-1231 "DNS query section"
            s["status"] = abi.ERR_MALFORMED
            return s, []
        entries.append(dict(section=abi.DNS_QUERY, flags8=0, off=start, type=_be16(m, pos), dns_class=_be16(m, pos + 2),
                            ttl=0, name=pos - start, data_len=0))
        pos += 4
    s["n_q"] = len(entries)
    for sec, declared, key in ((abi.DNS_ANSWER, s["an"], "n_an"), (abi.DNS_AUTHORITY, s["ns"], "n_ns"),
                               (abi.DNS_ADDITIONAL, s["ar"], "n_ar")):
        got = 0
        while got < declared and n - pos >= 12:  # DnsResponsePacket::from_buf_mut, dns.rs:904-945
            dl = _be16(m, pos + 10)
            room = n - pos - 12
            entries.append(dict(section=sec, flags8=abi.DNS_DATA_CUT if dl > room else 0, off=pos, type=_be16(m, pos + 2),
                                dns_class=_be16(m, pos + 4), ttl=_be16(m, pos + 6) << 16 | _be16(m, pos + 8),
                                name=_be16(m, pos), data_len=dl))
            pos += 12 + min(dl, room)
            got += 1
        s[key] = got
        if got < declared:
            s["flags8"] |= abi.DNS_SECTION_SHORT
    s["rest_off"] = pos
    return s, entries


def dns_frame_host(frame: bytes, rec, port: int = abi.DNS_PORT, any_udp: bool = False):
    """nexg_dns_batch for one frame and its record: (summary with msg_off,
    entries). Only the record's own fields decide whether it is a candidate."""
    flags, poff, plen = int(rec["flags"]), int(rec["payload_off"]), int(rec["payload_len"])
    port = port or abi.DNS_PORT
    cand = ((flags >> abi.STATUS_SHIFT) & 7 == 0 and flags & abi.L_UDP and plen > 0 and poff + plen <= len(frame) and
            (any_udp or int(rec["src_port"]) == port or int(rec["dst_port"]) == port))
    if not cand:
        return dict(dict.fromkeys(SUMMARY_FIELDS, 0), msg_off=0), []
    s, entries = dns_host(frame[poff:poff + plen])
    s["msg_off"] = poff if s["flags8"] & abi.DNS_CANDIDATE else 0
    return s, entries


# ---- views -------------------------------------------------------------------------
class DnsQuery:
    """DnsQueryPacket (dns.rs:615-620) over an entry of section 0."""

    def __init__(self, msg: bytes, e):
        off, name = int(e["off"]), int(e["name"])
        self.qname = msg[off:off + name]
        self.qtype = DnsType(e["type"])
        self.qclass = DnsClass(e["dns_class"])

    def qname_parsed(self) -> str:
        """dns.rs:718-720: decoded over the qname bytes alone, so a pointer
        indexes into the qname, not the message."""
        return decode_dns_name(self.qname, 0)[0]


class DnsResponse:
    """DnsResponsePacket (dns.rs:796-804) over an entry of section 1..3."""

    def __init__(self, msg: bytes, e):
        off = int(e["off"])
        self.name_tag = int(e["name"])
        self.rtype = DnsType(e["type"])
        self.rclass = DnsClass(e["dns_class"])
        self.ttl = int(e["ttl"])
        self.data_len = int(e["data_len"])
        self.data = msg[off + 12:off + 12 + min(self.data_len, len(msg) - off - 12)]

    def ip(self):
        """dns.rs:947-986."""
        if self.rtype == "A" and len(self.data) == 4:
            return ipaddress.IPv4Address(self.data)
        if self.rtype == "AAAA" and len(self.data) == 16:
            return ipaddress.IPv6Address(self.data)
        return None

    def dns_name(self) -> Optional[str]:
        """dns.rs:994-999: the record data decoded as a name of its own."""
        if self.rtype.name not in ("CNAME", "NS", "PTR"):
            return None
        try:
            return decode_dns_name(self.data, 0)[0]
        except DnsNameError:
            return None

    def txt_strings(self) -> Optional[List[str]]:
        """dns.rs:1007-1031."""
        if self.rtype != "TXT":
            return None
        pos, out = 0, []
        while pos < len(self.data):
            ln = self.data[pos]
            pos += 1
            if pos + ln > len(self.data):
                break
            try:
                out.append(self.data[pos:pos + ln].decode("utf-8"))
            except UnicodeDecodeError:
                return None
            pos += ln
        return out


class DnsPacket:
    """DnsPacket (dns.rs:1062-1069) over one frame's bytes, its nexg_dns
    summary and its nexg_dns_entry rows (n_q + n_an + n_ns + n_ar of them, in
    message order)."""

    def __init__(self, frame: bytes, summary, entries):
        if int(summary["status"]) != abi.FRAME_OK or not int(summary["flags8"]) & abi.DNS_CANDIDATE:
            raise ValueError("not a parsed DNS message")
        mo, ml = int(summary["msg_off"]), int(summary["msg_len"])
        self.msg = bytes(frame[mo:mo + ml])
        self.id = int(summary["id"])
        f = self.flags = int(summary["flags"])
        self.is_response = f >> 15 & 1
        self.opcode = OpCode(f >> 11 & 0xF)
        self.is_authoriative = f >> 10 & 1
        self.is_truncated = f >> 9 & 1
        self.is_recursion_desirable = f >> 8 & 1
        self.is_recursion_available = f >> 7 & 1
        self.zero_reserved = f >> 6 & 1
        self.is_answer_authenticated = f >> 5 & 1
        self.is_non_authenticated_data = f >> 4 & 1
        self.rcode = RetCode(f & 0xF)
        self.query_count, self.response_count = int(summary["qd"]), int(summary["an"])
        self.authority_rr_count, self.additional_rr_count = int(summary["ns"]), int(summary["ar"])
        by = {k: [e for e in entries if int(e["section"]) == k] for k in range(4)}
        self.queries = [DnsQuery(self.msg, e) for e in by[abi.DNS_QUERY]]
        self.responses = [DnsResponse(self.msg, e) for e in by[abi.DNS_ANSWER]]
        self.authorities = [DnsResponse(self.msg, e) for e in by[abi.DNS_AUTHORITY]]
        self.additionals = [DnsResponse(self.msg, e) for e in by[abi.DNS_ADDITIONAL]]
        self.payload = self.msg[int(summary["rest_off"]):]


def frame_entries(dns, tile_first, entries, i):
    """Frame i's rows of a nexg_dns_entries output (host arrays)."""
    s = dns[i]
    k = int(s["n_q"]) + int(s["n_an"]) + int(s["n_ns"]) + int(s["n_ar"])
    first = int(tile_first[i >> 8]) + int(s["first"])
    return entries[first:first + k]
