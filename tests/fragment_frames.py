"""Fragmentation test traffic (include/nexg.h nexg_fragment_plan /
nexg_fragment_frames): the corpus, and an independent reassembly. Nothing here
comes from nex_amd.fragment: frames are assembled by hand, checksums are
tests.helpers.rfc1071, and reassemble() puts pieces back together the way a
receiving host would (RFC 791 section 3.2, "An Example Reassembly Procedure"),
so a fault shared by the kernel and its Python restatement still shows."""
import functools

import numpy as np

from tests.helpers import rfc1071

MTUS = (68, 576, 1280, 1500, 9000)
ETH = bytes.fromhex("02a0b0c0d0e1") + bytes.fromhex("02a0b0c0d0e2")
SRC, DST = bytes([192, 0, 2, 1]), bytes([198, 51, 100, 7])

# IPv4 options by what the fragments behind the first do with them
RA = bytes([0x94, 4, 0, 0])                                 # router alert: copied
LSRR = bytes([0x83, 7, 4, 10, 0, 0, 9])                     # loose source route: copied
RR = bytes([0x07, 11, 4, 1, 2, 3, 4, 5, 6, 7, 8])           # record route: not copied
TS = bytes([0x44, 12, 5, 0, 9, 9, 9, 9, 8, 8, 8, 8])        # timestamp: not copied
OPTIONS = {
    "copied": RA,
    "not copied": TS,
    "copied, nop, not copied": LSRR + b"\x01" + RR + b"\x01",
    "nop run then not copied": b"\x01" * 5 + RR,
    "eol in the middle": RA + b"\x00" + RR,                 # what follows the EOL stays as it is
    "length 0": RA + bytes([0x44, 0, 9, 9]),                # the walk stops: the rest stays
    "length 1": bytes([0x07, 1, 9, 9]) + RA,
    "length overruns": RA + bytes([0x07, 5, 1, 2]),         # 5 bytes declared, 4 left
    "type in the last byte": RA + b"\x01\x01\x01\x07",      # no length byte
    "length reaches the end exactly": RA + bytes([0x07, 8, 4, 1, 2, 3, 4, 5]),
    "forty bytes": RR + b"\x01" + LSRR + b"\x01\x01" + TS + RA + b"\x00" + b"\xEE\x07",
    "forty bytes that re-serialise to themselves": RR + b"\x01" + LSRR + b"\x01\x01" + TS + RA + b"\x01\x01\x01",
}
assert all(len(o) % 4 == 0 and len(o) <= 40 for o in OPTIONS.values())
assert len(OPTIONS["forty bytes"]) == len(OPTIONS["forty bytes that re-serialise to themselves"]) == 40


def pattern(n, seed=0):
    """n bytes with no period of 2, 4, 8 or 16 (a piece cut at the wrong place shows)."""
    i = np.arange(n, dtype=np.uint32)
    return ((i * 131 + (i >> 8) * 17 + seed * 29 + 7) & 0xFF).astype(np.uint8).tobytes()


def be(v, n=2):
    return int(v).to_bytes(n, "big")


def ipv4(data_len, opts=b"", proto=17, word=0, ident=0xBEEF, tos=0x2E, ttl=61, trailer=0, seed=0, total=None, first=0x40,
         ethertype=0x0800):
    """An Ethernet / IPv4 frame with `data_len` bytes behind the header: a UDP or
    TCP header in front of a pattern (a plain pattern when there is no room, or
    for a later fragment). word: the flags / fragment offset word. `first`: the
    version nibble in the high half; the IHL comes from the options. total:
    the total length field when it is to differ from the bytes there."""
    hl = 20 + len(opts)
    data = pattern(data_len, seed + data_len)
    if not word & 0x1FFF and proto == 17 and data_len >= 8:
        data = be(1234) + be(53) + be(data_len) + be(0) + data[8:]
    elif not word & 0x1FFF and proto == 6 and data_len >= 20:
        data = be(4321) + be(80) + be(7, 4) + be(9, 4) + bytes([0x50, 0x18]) + be(512) + be(0) + be(0) + data[20:]
    h = bytearray(bytes([first | hl // 4, tos]) + be(hl + data_len if total is None else total) + be(ident) + be(word) +
                  bytes([ttl, proto, 0, 0]) + SRC + DST + opts)
    h[10:12] = be(rfc1071(bytes(h)))
    return ETH + be(ethertype) + bytes(h) + data + pattern(trailer, 77)


def ipv6(payload_len, declared=None, first=0x60):
    return (ETH + b"\x86\xdd" + bytes([first, 0x12, 0x34, 0x56]) + be(payload_len if declared is None else declared) +
            bytes([17, 64]) + bytes(range(16)) + bytes(range(16, 32)) + pattern(payload_len, 5))


@functools.lru_cache(maxsize=None)
def corpus():
    """[(name, frame or None)]: None is an extent outside the data."""
    c = []
    # every option shape, long enough to split at every mtu up to 1500 (three pieces and more)
    for k, (name, o) in enumerate(OPTIONS.items()):
        c.append((f"options: {name}", ipv4(3000 + k, o, proto=(17, 6)[k % 2], seed=k)))
    c.append(("options: forty bytes, splits at 9000", ipv4(20001, OPTIONS["forty bytes"], proto=6)))
    c.append(("options: mixed, splits at 9000", ipv4(18003, OPTIONS["copied, nop, not copied"])))
    # header lengths 20 / 24 / 60, UDP and TCP
    for proto in (17, 6):
        for o in (b"", RA, OPTIONS["forty bytes"]):
            c.append((f"hl {20 + len(o)} proto {proto}", ipv4(2500 + len(o), o, proto=proto, seed=proto)))
    # inputs that are fragments already, DF, the reserved bit
    c.append(("fragment: first of a train (MF)", ipv4(2960, word=0x2000)))
    c.append(("fragment: middle (MF, offset 370)", ipv4(2960, RA, word=0x2000 | 370)))
    c.append(("fragment: last (offset 740)", ipv4(1931, TS, word=740)))
    c.append(("fragment: last, splits at 9000", ipv4(19000, word=1000)))
    c.append(("DF set", ipv4(2000, word=0x4000)))
    c.append(("DF set, options", ipv4(3001, OPTIONS["copied, nop, not copied"], word=0x4000)))
    c.append(("DF set, splits at 9000", ipv4(9100, word=0x4000)))
    c.append(("DF and MF set, an offset", ipv4(2000, word=0x6000 | 11)))
    c.append(("DF set and it fits everywhere", ipv4(40, word=0x4000)))
    c.append(("reserved bit set", ipv4(2222, word=0x8000)))
    c.append(("reserved bit, DF and MF set", ipv4(2223, RA, word=0xE000 | 5)))
    c.append(("Ethernet padding behind the IP bytes", ipv4(1999, trailer=7)))
    c.append(("Ethernet padding, fits", ipv4(26, trailer=6)))
    c.append(("Ethernet padding, 60 bytes of options", ipv4(4000, OPTIONS["forty bytes"], trailer=15)))
    # the edges of every mtu: TL at mtu - 1, mtu, mtu + 1; D at p, p +- 1, 2p, 2p +- 1
    for m in MTUS:
        for tl in (m - 1, m, m + 1):
            c.append((f"mtu {m}: TL {tl}", ipv4(tl - 20, seed=m)))
        for o in (b"", RA):
            hl = 20 + len(o)
            p = (m - hl) & ~7
            for d in (p - 1, p, p + 1, 2 * p - 1, 2 * p, 2 * p + 1):
                c.append((f"mtu {m} hl {hl}: D {d}", ipv4(d, o, seed=d)))
    for d in (8, 9, 16, 17):
        c.append((f"mtu 68 hl 60: D {d}", ipv4(d, OPTIONS["forty bytes"], seed=d)))
    c.append(("mtu 68 hl 60, options that re-serialise: D 17", ipv4(17, OPTIONS["forty bytes that re-serialise to themselves"])))
    c.append(("hl 60, options that re-serialise, splits at 9000", ipv4(9500, OPTIONS["forty bytes that re-serialise to themselves"], proto=6)))
    # the fragment offset's 13 bits: at mtu 576 and hl 20 six pieces step 69 units each
    c.append(("offset ends at 8191 exactly at mtu 576", ipv4(3000, word=8191 - 5 * 69)))
    c.append(("offset overflows by one at mtu 576", ipv4(3000, word=8191 - 5 * 69 + 1)))
    c.append(("offset 8000 overflows below mtu 9000", ipv4(3000, word=0x2000 | 8000)))
    # the longest frames a table holds
    c.append(("65535 bytes, hl 20", ipv4(65535 - 34)))
    c.append(("65535 bytes, hl 60", ipv4(65535 - 74, OPTIONS["forty bytes"], proto=6)))
    # not IPv4, one cause each, every one longer than most mtus
    c.append(("not IPv4: EtherType 0x1234", ipv4(2000, ethertype=0x1234)))
    c.append(("not IPv4: 33 bytes", ipv4(0)[:33]))
    c.append(("IPv4 of 34 bytes", ipv4(0)))
    c.append(("not IPv4: version 5", ipv4(2000, first=0x50)))
    c.append(("not IPv4: IHL 4", bytes(ipv4(2000)[:14]) + b"\x44" + ipv4(2000)[15:]))
    c.append(("not IPv4: IHL 15 in 60 bytes", bytes(ipv4(26)[:14]) + b"\x4F" + ipv4(26)[15:]))
    c.append(("not IPv4: total length below the header", ipv4(2000, total=19)))
    c.append(("not IPv4: total length one past the frame", ipv4(2000, total=2021)))
    c.append(("total length ends the frame exactly", ipv4(2000, total=2020)))
    c.append(("VLAN-tagged IPv4", ETH + b"\x81\x00\x00\x64" + ipv4(2000)[12:]))
    c.append(("ARP", ETH + b"\x08\x06" + bytes([0, 1, 8, 0, 6, 4, 0, 1]) + ETH[6:] + SRC + bytes(6) + DST))
    # IPv6: never fragmented
    c.append(("IPv6 under every mtu", ipv6(20)))
    c.append(("IPv6 at 68 exactly", ipv6(28)))
    c.append(("IPv6 one over 68", ipv6(29)))
    c.append(("IPv6 over 1500", ipv6(3000)))
    c.append(("IPv6 over 9000", ipv6(9001)))
    c.append(("IPv6 payload length past the frame", ipv6(3000, declared=3001)))
    c.append(("IPv6 EtherType, version 5", ipv6(3000, first=0x50)))
    c.append(("IPv6 EtherType, 53 bytes", ipv6(0)[:53]))
    c.append(("IPv6 with padding, over 1280", ipv6(1300) + bytes(9)))
    # no Ethernet header, and extents the table does not hold
    c.append(("empty", b""))
    c.append(("13 bytes", ETH + b"\x08"))
    c.append(("14 bytes", ETH + b"\x08\x00"))
    c.append(("bad extent", None))
    c.append(("a second bad extent", None))
    return tuple(c)


def frames():
    return [f for _, f in corpus()]


def small(limit=4096):
    """The indices of the corpus frames under `limit` bytes (bad extents included)."""
    return [i for i, (_, f) in enumerate(corpus()) if f is None or len(f) < limit]


# ---- the receiving host ----------------------------------------------------------------------

def later_options_ref(opts: bytes) -> bytes:
    """What RFC 791 leaves of an option list in the fragments behind the first
    when the header keeps its length: an option without the copied flag (bit 7
    of its type) is overwritten with No Operation."""
    out = list(opts)
    at = 0
    while at < len(opts) and opts[at] != 0:
        if opts[at] == 1:
            at += 1
            continue
        room = len(opts) - at
        if room < 2 or not 2 <= opts[at + 1] <= room:
            break
        size = opts[at + 1]
        if opts[at] < 0x80:
            out[at:at + size] = [1] * size
        at += size
    return bytes(out)


class Piece:
    def __init__(self, frame: bytes):
        assert len(frame) >= 34 and frame[12:14] == b"\x08\x00" and frame[14] >> 4 == 4, "a piece is an IPv4 frame"
        self.eth = frame[:14]
        self.hl = 4 * (frame[14] & 15)
        self.header = frame[14:14 + self.hl]
        self.total = int.from_bytes(frame[16:18], "big")
        assert len(frame) == 14 + self.total, "a piece ends with its IP bytes: no padding, nothing dropped"
        assert rfc1071(self.header) == 0, "a piece's header checksum verifies"
        word = int.from_bytes(frame[20:22], "big")
        self.flags, self.offset = word & 0xC000, word & 0x1FFF
        self.more = bool(word & 0x2000)
        self.data = frame[14 + self.hl:]


def reassemble(pieces, first_offset=0, last_more=False):
    """The datagram the pieces (frames, in any order) came from, as a frame:
    sorted by offset, contiguous from `first_offset`, every piece but the last a
    multiple of 8 bytes with MF set, the last with MF == last_more; the fields
    that fragments share are equal, the later pieces' options are the first's
    under later_options_ref. The header is the first piece's with the total
    length, the original's MF and offset, and the checksum put back."""
    ps = sorted((Piece(bytes(p)) for p in pieces), key=lambda p: p.offset)
    assert ps, "no piece"
    head = ps[0]
    at = first_offset
    for k, p in enumerate(ps):
        assert p.offset == at, f"piece {k} starts at unit {p.offset}, the data so far ends at {at}"
        assert p.eth == head.eth and p.hl == head.hl and p.flags == head.flags, f"piece {k}: Ethernet, IHL, reserved or DF differ"
        assert p.header[:2] == head.header[:2] and p.header[4:6] == head.header[4:6], f"piece {k}: TOS or id differ"
        assert p.header[8:10] == head.header[8:10] and p.header[12:20] == head.header[12:20], f"piece {k}: TTL, protocol or addresses differ"
        if k:
            assert p.header[20:] == later_options_ref(head.header[20:]), f"piece {k}: options"
        if k + 1 < len(ps):
            assert p.more and len(p.data) % 8 == 0 and len(p.data) > 0, f"piece {k}: MF clear or data not a multiple of 8"
            at += len(p.data) // 8
        else:
            assert p.more == last_more, "the last piece carries the original's MF"
    data = b"".join(p.data for p in ps)
    h = bytearray(head.header)
    h[2:4] = be(head.hl + len(data))
    h[6:8] = be(head.flags | (0x2000 if last_more else 0) | first_offset)
    h[10:12] = b"\0\0"
    h[10:12] = be(rfc1071(bytes(h)))
    return head.eth + bytes(h) + data


def datagram(frame: bytes, clear_df=False):
    """What reassemble must give back for an input frame: its bytes up to the
    end of the IP datagram, DF cleared when the pieces were made under
    IGNORE_DF, the header checksum as rfc1071 gives it."""
    hl, total = 4 * (frame[14] & 15), int.from_bytes(frame[16:18], "big")
    h = bytearray(frame[14:14 + hl])
    if clear_df:
        h[6] &= 0xBF
    h[10:12] = b"\0\0"
    h[10:12] = be(rfc1071(bytes(h)))
    return frame[:14] + bytes(h) + frame[14 + hl:14 + total]
