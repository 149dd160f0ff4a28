"""Seeded fuzz corpora for the four second passes (DNS, decap, select, flow).

Every generator is deterministic from its seed and builds frames with the
builders of dns_frames.py, tunnel_frames.py, select_frames.py and
flow_frames.py. The hand corpora of those modules cover the shapes (counts,
layouts, alignments); these cover the content: structured random messages and
headers, explicit boundary families (a length that ends exactly on, one before
and one past a limit), then byte rewrites and helpers.mutate_frames.

The check_* functions assert, from the independent reference
(second_pass_ref.py) alone, that a corpus really exercises the walks: a sweep
cannot pass on a corpus that says nothing. tests/test_second_pass_ref.py,
test_second_pass_mutants.py and test_gpu_second_pass_fuzz.py share the corpora
through corpora() (built once per process)."""
import functools
import itertools

import numpy as np

from nex_amd import abi
from nex_amd.flow import DEFAULT_KEY
from nex_amd.select import Filter, Rule
from tests import dns_frames as df
from tests import flow_frames as ff
from tests import helpers
from tests import second_pass_ref as ref
from tests import select_frames as sf
from tests import tunnel_frames as tf

SEED = 20261020
DNS_PARSE_FLAGS = abi.PARSE_VLAN           # the DNS and decap tests parse with the VLAN extension
SELECT_PARSE_FLAGS = sf.PARSE_FLAGS        # the select and flow tests add strict mode


def _rnd(rng, n) -> bytes:
    return bytes(rng.integers(0, 256, max(0, int(n)), dtype=np.uint8))


def oracle_records(oracle, frames, flags=0, ip_offset=0):
    """The oracle's records of a list of frames, parsed as one packed batch."""
    offs = np.zeros(len(frames) + 1, np.uint64)
    offs[1:] = np.cumsum([len(f) for f in frames])
    data = np.frombuffer(b"".join(frames) + bytes(16), np.uint8)
    return oracle.parse_packed(data, offsets=offs, flags=flags, ip_offset=ip_offset)


# ---- DNS ---------------------------------------------------------------------------------------

def _rr(rng, data=None, dl=None, tag=None):
    """A resource record: name_tag, type, class, ttl, data_len, data."""
    data = _rnd(rng, rng.integers(0, 20)) if data is None else data
    dl = len(data) if dl is None else dl
    tag = (0xC00C if rng.random() < 0.5 else int(rng.integers(0, 1 << 16))) if tag is None else tag
    rtype = int(rng.choice([1, 28, 5, 16, 2, 41, int(rng.integers(0, 1 << 16))]))
    return (tag.to_bytes(2, "big") + rtype.to_bytes(2, "big") + int(rng.integers(0, 5)).to_bytes(2, "big") +
            int(rng.integers(0, 1 << 32)).to_bytes(4, "big") + dl.to_bytes(2, "big") + data)


def _query(rng):
    """A query: labels of 0..63 bytes, now and then a length byte >= 0xC0 (a
    plain length to this walk) with or without its bytes, type and class."""
    out = b""
    for _ in range(int(rng.integers(0, 4))):
        k = rng.random()
        ln = (63 if k < 0.06 else int(rng.integers(0xC0, 0x100)) if k < 0.14 else int(rng.integers(0, 64)) if k < 0.2
              else int(rng.integers(1, 10)))
        present = ln if ln < 0xC0 or rng.random() < 0.35 else int(rng.integers(0, 6))
        out += bytes([ln]) + _rnd(rng, present)
        if ln == 0:
            break
    else:
        out += b"\0"
    return out + int(rng.choice([1, 28, 255, 33])).to_bytes(2, "big") + int(rng.integers(1, 5)).to_bytes(2, "big")


def _declared(rng, present):
    return max(0, present + int(rng.choice([0, 0, 0, 0, -1, 1, 2, 65535 - present])))


def structured_message(rng):
    """qd 0..3 queries and 0..4 records per section; data_len below, equal to
    and above what is left; declared counts below, equal to and above the
    counts present (65535 included)."""
    present = [int(rng.integers(0, 4))] + [int(rng.integers(0, 5)) if rng.random() < 0.6 else 0 for _ in range(3)]
    body = b"".join(_query(rng) for _ in range(present[0]))
    nrec = sum(present[1:])
    for k in range(nrec):
        data = _rnd(rng, rng.integers(0, 20))
        d = int(rng.choice([0, 0, 0, 0, -1, 1, 3, 300, 65535])) if k == nrec - 1 or rng.random() < 0.15 else 0
        body += _rr(rng, data, min(65535, max(0, len(data) + d)))
    tail = _rnd(rng, rng.integers(0, 14)) if rng.random() < 0.3 else b""
    return df.header(int(rng.integers(0, 1 << 16)), int(rng.integers(0, 1 << 16)),
                     *[_declared(rng, p) for p in present]) + body + tail


def boundary_messages(rng):
    """The explicit boundary families (see the module docstring of
    tests/test_second_pass_mutants.py for what each one kills)."""
    out = []
    q = df.qname("ab.example") + b"\x00\x01\x00\x01"
    a4 = bytes([192, 0, 2, 9])
    # a label ending on the message's last byte; the terminator and 0..4 bytes after it
    for labels in ([5], [3, 7], [63], [1], [2, 1, 1]):
        name = b"".join(bytes([n]) + _rnd(rng, n) for n in labels)
        for qd, lead in ((1, b""), (2, q)):
            out.append(df.header(0x4C01, 0x0100, qd) + lead + name)            # the last label's last byte ends it
            out.append(df.header(0x4C02, 0x0100, qd) + lead + name[:-1])        # one byte short of that
            for t in range(5):
                out.append(df.header(0x4C03, 0x0100, qd) + lead + name + b"\0" + _rnd(rng, t))
    # exactly 11, 12 and 13 bytes left before a declared record, in each section
    for left in (11, 12, 13):
        for counts in ((2, 0, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1), (0, 1, 0), (0, 0, 1), (65535, 0, 0)):
            for lead in (q, b""):
                rec = _rr(rng, a4) if counts[0] else b""
                out.append(df.header(0x4C10 + left, 0x8180, 1 if lead else 0, *counts) + lead + rec + _rnd(rng, left))
    # data_len equal to the room, one below and one above it
    for room in (0, 1, 2, 5, 20):
        for d in (-1, 0, 1):
            if room + d < 0:
                continue
            for counts in ((1, 0, 0), (2, 0, 0), (1, 1, 0), (0, 0, 1)):
                out.append(df.header(0x4C20, 0x8180, 1, *counts) + q + _rr(rng, _rnd(rng, room), room + d))
                out.append(df.header(0x4C21, 0x8180, 1, *counts) + q + _rr(rng, a4) + _rr(rng, _rnd(rng, room), room + d))
    # a failing second query after a good first one
    for second in (b"", b"\x05ab", df.qname("x") + b"\x00\x01\x00", b"\xc0\x0c\x00\x01\x00\x01", b"\x3f" + bytes(62),
                   df.qname("ok") + b"\x00\x01\x00\x01"):
        out.append(df.header(0x4C30, 0x0100, 2) + q + second)
        out.append(df.header(0x4C31, 0x0100, 3, 1) + q + second + _rr(rng, a4))
    # each section alone short: the records present equal the declared counts but in one section
    for sec in range(3):
        for tail in (0, 1, 11):
            present = [1, 1, 1]
            for k in range(sec, 3):  # nothing is present from the short section on
                present[k] = 0
            declared = [1 if k < sec else 0 for k in range(3)]
            declared[sec] = 1
            body = b"".join(_rr(rng, a4) for _ in range(sum(present)))
            out.append(df.header(0x4C40 + sec, 0x8180, 1, *declared) + q + body + _rnd(rng, tail))
            declared[sec] = 2  # one of two present
            out.append(df.header(0x4C48 + sec, 0x8180, 1, *declared) + q + body + _rr(rng, a4) + _rnd(rng, tail))
    return out


def dns_messages(seed=SEED, structured=500, truncated_seeds=64, rewrites=600):
    """(messages, count of truncation seeds used): every family, before wrapping."""
    rng = np.random.default_rng(seed)
    base = [structured_message(rng) for _ in range(structured)]
    out = list(base)
    seeds = [m for m in base if 24 <= len(m) <= 72][:truncated_seeds]
    assert len(seeds) >= 64
    for m in seeds:  # truncate at every byte position
        out += [m[:k] for k in range(len(m))]
    bound = boundary_messages(rng)
    out += bound
    pool = base + bound
    for _ in range(rewrites):  # single-byte rewrites inside the message
        m = bytearray(pool[int(rng.integers(len(pool)))])
        if not m:
            continue
        k = rng.random()
        if k < 0.3 and len(m) >= 12:     # a declared count
            m[int(rng.integers(4, 12))] = int(rng.choice([0, 1, 2, 255]))
        elif k < 0.6 and len(m) > 12:    # a small value somewhere in the body: a length byte, a data_len byte
            m[int(rng.integers(12, len(m)))] = int(rng.integers(0, 24))
        else:
            m[int(rng.integers(len(m)))] = int(rng.integers(256))
        out.append(bytes(m))
    return out, len(seeds)


def wrap_dns(msg: bytes, i: int) -> bytes:
    """Eth/IPv4/UDP to port 53, Eth/IPv6/UDP from port 53, or VLAN-tagged."""
    k = i % 3
    if k == 0:
        return df.wrap(msg, df.CLIENT, 53, False)
    if k == 1:
        return df.wrap(msg, 53, df.CLIENT, True)
    return helpers.vlan(df.wrap(msg, df.CLIENT, 53, i % 2 == 0), [0x0064 + i % 7])


def dns_frames(seed=SEED, mutated=400):
    msgs, _ = dns_messages(seed)
    frames = [wrap_dns(m, i) for i, m in enumerate(msgs)]
    rng = np.random.default_rng(seed + 1)
    small = [f for f in frames if len(f) < 200]
    return frames + helpers.mutate_frames(rng, small, mutated)


def check_dns(frames, recs):
    """The corpus conditions, from the independent reference alone."""
    n = len(frames)
    walks = ok = bad = short = cut = label_end = 0
    first_short = set()
    for f, r in zip(frames, recs):
        s, rows = ref.dns_frame_rows(f, r)
        msg = ref.udp_payload(f, r)
        if s["flags8"] & abi.DNS_CANDIDATE:
            walks += 1
            ok += s["status"] == abi.FRAME_OK
            bad += s["status"] == abi.ERR_MALFORMED
            first_short.add(ref.first_short_section(msg))
            cut += any(e["flags8"] & abi.DNS_DATA_CUT for e in rows)
            label_end += ref.qname_label_ends_message(msg)
        short += s["status"] == abi.ERR_BUFFER_TOO_SHORT
    assert walks >= 0.6 * n, (walks, n)
    assert min(ok, bad, short) >= 0.05 * n, (ok, bad, short, n)
    assert {1, 2, 3} <= first_short, first_short
    assert cut > 0 and label_end > 0, (cut, label_end)
    return dict(frames=n, walks=walks, ok=ok, malformed=bad, too_short=short, data_cut=cut, label_end=label_end)


# ---- tunnels ------------------------------------------------------------------------------------

CUSTOM_VXLAN_PORT = 4790


def _carrier_ip(payload, proto, k):
    """Over IPv4, over IPv6, VLAN-tagged."""
    k %= 3
    if k == 2:
        return helpers.vlan(tf.outer_ip(payload, proto, False), [0x0123])
    return tf.outer_ip(payload, proto, k == 1)


def _carrier_udp(payload, port, k):
    k %= 3
    if k == 2:
        return helpers.vlan(tf.outer_udp(payload, port, True), [0x0045])
    return tf.outer_udp(payload, port, k == 1)


def _gre_header(rng, c, r, k, s, rest, proto):
    """The first word with the given C/R/K/S bits and `rest` in the low 12 bits
    (strict source route, recursion control, reserved, version), then every
    optional field the bits call for, each a random word."""
    flags = c << 15 | r << 14 | k << 13 | s << 12 | rest
    h = flags.to_bytes(2, "big") + proto.to_bytes(2, "big")
    return h + _rnd(rng, 4 * ((c | r) + k + s))


def tunnel_frames(seed=SEED):
    rng = np.random.default_rng(seed + 2)
    eth, ip4, ip6 = tf.inner_sets()
    eth = [f for f in eth if f]
    inner_of = {0x6558: eth, 0x0800: ip4, 0x86DD: ip6, 0x880B: [_rnd(rng, n) for n in (1, 7, 30)]}
    out = []
    j = 0
    for c, r, k, s in itertools.product((0, 1), repeat=4):
        for rest in (0, None):
            for proto in (0x6558, 0x0800, 0x86DD, 0x880B):
                low = 0 if rest == 0 else int(rng.integers(1, 1 << 12))
                h = _gre_header(rng, c, r, k, s, low, proto)
                for n in range(len(h) + 2):  # payload length 0 .. header length + 1
                    out.append(_carrier_ip((h + _rnd(rng, 1))[:n], 47, j))
                    j += 1
                for _ in range(3):  # and with a whole inner frame behind the header
                    inner = inner_of[proto]
                    h = _gre_header(rng, c, r, k, s, low, proto)
                    out.append(_carrier_ip(h + inner[int(rng.integers(len(inner)))], 47, j))
                    j += 1
    for i in range(700):  # VXLAN: random flag byte and reserved fields, payload 0..9 B and longer
        h = _rnd(rng, 8)
        port = CUSTOM_VXLAN_PORT if i % 7 == 6 else abi.VXLAN_PORT  # 7: every payload length meets both ports
        if i % 3 == 0:
            body = (h + _rnd(rng, 1))[: i // 3 % 10]
        else:
            body = h + eth[int(rng.integers(len(eth)))]
        out.append(_carrier_udp(body, port, i))
    plain = [f for f in helpers.crafted_frames() if f] + [c.frame for c in tf.cases() if c.kind == abi.TUN_NONE]
    out += helpers.mutate_frames(rng, plain, 150)
    small = [f for f in out if len(f) < 200]
    return out + helpers.mutate_frames(rng, small, 250)


def check_decap(frames, recs, vxlan_port=abi.VXLAN_PORT):
    n = len(frames)
    cand = accepted = malformed = 0
    took, refused = set(), set()
    for f, r in zip(frames, recs):
        kind = ref.tunnel_candidate(f, r, vxlan_port=vxlan_port)
        if kind == abi.TUN_NONE:
            continue
        cand += 1
        t, _, ilen = ref.decap_frame(f, r, vxlan_port=vxlan_port)
        good = t["status"] == abi.FRAME_OK
        accepted += good
        malformed += not good
        if kind == abi.TUN_GRE and int(r["payload_len"]) >= 1:
            crks = f[int(r["payload_off"])] >> 4
            (took if good else refused).add(crks)
    assert cand >= 0.7 * n, (cand, n)
    assert accepted >= 0.2 * n and malformed >= 0.2 * n, (accepted, malformed, n)
    without_r = {x for x in range(16) if not x & 4}
    assert without_r <= took and (set(range(16)) - without_r) <= refused, (sorted(took), sorted(refused))
    assert not took & (set(range(16)) - without_r)
    return dict(frames=n, candidates=cand, accepted=accepted, malformed=malformed)


# ---- select --------------------------------------------------------------------------------------

TCP_CWR, TCP_ECE = 0x80, 0x40
Y6 = "2001:db8:aaaa:bbbb:cccc:dddd:eeee:fff0"  # X6 but for its last word


def added_frames():
    """Frames the select and flow hand corpora lack: TCP with CWR / ECE, IPv6
    frames that end exactly with the fixed header, IPv4 first, middle and last
    fragments whose payload parses as TCP and as UDP."""
    P = bytes(range(24))
    out = []
    for fl in (TCP_CWR | sf.TCP_SYN, TCP_ECE | sf.TCP_ACK, TCP_CWR | TCP_ECE | sf.TCP_SYN, 0xFF, TCP_CWR, TCP_ECE):
        out.append(sf._v4("tcp", sf.A4, sf.B4, 40010, 443, "", fl, P).frame)
        out.append(sf._v6("tcp", sf.A6, sf.B6, 40011, 443, "", fl, P).frame)
    bare = sf.eth(sf.ip6(sf.A6, sf.B6, 59, b""), 0x86DD)  # next header 59 (none), payload length 0
    out += [bare, sf.eth(sf.ip6(sf.X6, sf.C6, 59, b""), 0x86DD), helpers.vlan(bare, [0x0064])]
    for l4, proto in (("tcp", 6), ("udp", 17)):
        seg = (sf.tcp_seg(sf.A4, sf.B4, 3333, 4444, sf.TCP_ACK, P) if l4 == "tcp"
               else sf.udp_dgram(sf.A4, sf.B4, 3333, 4444, P))
        for mf, off in ((True, 0), (True, 3), (False, 3), (False, 0x1FFF), (False, 1)):
            out.append(sf.eth(ff.ip4_frag(sf.A4, sf.B4, proto, seg, mf=mf, frag_off=off)))
            out.append(sf.eth(ff.ip4_frag(sf.B4, sf.A4, proto, seg, mf=mf, frag_off=off)))
    return out


def select_frames(seed=SEED, mutated=700):
    """(frames, count of the leading mutated ones): helpers.mutate_frames over
    the select corpus, then the corpus itself and added_frames()."""
    rng = np.random.default_rng(seed + 3)
    base = [x.frame for x in sf.small_corpus() if not x.junk and len(x.frame) < 2000] + added_frames()
    return helpers.mutate_frames(rng, base, mutated) + base, mutated


def check_status_ok(recs, mutated):
    ok = int(((recs["flags"][:mutated] >> abi.STATUS_SHIFT) & 7 == 0).sum())
    assert ok >= 0.5 * mutated, (ok, mutated)
    return ok


def _valid_test_combinations():
    """Every `tests` value nexg_select_batch accepts."""
    out = []
    for t in range(abi.RULE_ALL + 1):
        if t & abi.RULE_ANY_PORT and t & (abi.RULE_SRC_PORT | abi.RULE_DST_PORT):
            continue
        if t & abi.RULE_ANY_ADDR and t & (abi.RULE_SRC_ADDR | abi.RULE_DST_ADDR):
            continue
        out.append(t)
    return out


def _flip(addr: bytes, bit: int) -> bytes:
    """`addr` with bit `bit` (0 = the most significant) inverted."""
    b = bytearray(addr)
    b[bit // 8] ^= 0x80 >> (bit % 8)
    return bytes(b)


def _rule_address(rng, addr: bytes, bits: int):
    """The frame's own address, flipped in exactly bit bits - 1 (the last
    prefix bit: no match), bit `bits` (the first bit past the prefix: still a
    match) or not at all."""
    k = int(rng.integers(3))
    if k == 0 and bits >= 1:
        addr = _flip(addr, bits - 1)
    elif k == 1 and bits < 8 * len(addr):
        addr = _flip(addr, bits)
    return addr + bytes(16 - len(addr))


def random_rule(rng, tests, frame, rec):
    """A rule with the given tests whose values come from one corpus frame:
    range ends at the frame's value +- 1, prefixes around the frame's own
    addresses, tcp_mask / tcp_value over all 8 bits."""
    r = Rule(tests=tests)
    fl = int(rec["flags"])
    if rng.random() < 0.3:
        m = int(rng.choice([abi.L_TCP, abi.L_UDP, abi.L_IPV4, abi.L_IPV6, abi.L_VLAN, abi.L_TCP | abi.L_UDP,
                            7 << abi.STATUS_SHIFT, abi.C_L4_CHECKED | abi.C_L4_OK]))
        r.flags_mask, r.flags_value = m, fl & m if rng.random() < 0.8 else m
    if tests & abi.RULE_PROTO:
        r.ip_proto = int(rec["ip_proto"]) if rng.random() < 0.8 else int(rng.choice([6, 17, 1, 58, 47]))

    def span(v, top=65535):
        lo = min(top, max(0, v + int(rng.integers(-1, 2)) - int(rng.choice([0, 0, 1, 1000]))))
        hi = min(top, max(lo, v + int(rng.integers(-1, 2)) + int(rng.choice([0, 0, 1, 1000]))))
        return lo, hi

    sp, dp = int(rec["src_port"]), int(rec["dst_port"])
    if tests & abi.RULE_SRC_PORT:
        r.sport_lo, r.sport_hi = span(sp)
    if tests & abi.RULE_DST_PORT:
        r.dport_lo, r.dport_hi = span(dp)
    if tests & abi.RULE_ANY_PORT:
        r.sport_lo, r.sport_hi = span(sp if rng.random() < 0.5 else dp)
    if tests & abi.RULE_LENGTH:
        r.len_lo, r.len_hi = span(len(frame))
    if tests & abi.RULE_TCP_FLAGS:
        r.tcp_mask = int(rng.integers(0, 256))
        r.tcp_value = int(rec["l4_type"]) & r.tcp_mask
        if rng.random() < 0.3:
            r.tcp_value = int(rng.integers(0, 256)) & r.tcp_mask
    if tests & (abi.RULE_SRC_ADDR | abi.RULE_DST_ADDR | abi.RULE_ANY_ADDR):
        a = ref.frame_addresses(frame, rec, len(frame), 6) or ref.frame_addresses(frame, rec, len(frame), 4)
        if a is None:
            a = (_rnd(rng, 4), _rnd(rng, 4)) if rng.random() < 0.5 else (_rnd(rng, 16), _rnd(rng, 16))
        r.family = 4 if len(a[0]) == 4 else 6
        width = 8 * len(a[0])
        pick = lambda: int(rng.choice([0, 1, width - 1, width, int(rng.integers(0, width + 1)),  # noqa: E731
                                       int(rng.integers(0, width + 1))]))
        if tests & abi.RULE_SRC_ADDR:
            r.src_bits = pick()
            r.src = _rule_address(rng, a[0], r.src_bits)
        if tests & abi.RULE_DST_ADDR:
            r.dst_bits = pick()
            r.dst = _rule_address(rng, a[1], r.dst_bits)
        if tests & abi.RULE_ANY_ADDR:
            r.src_bits = pick()
            r.src = _rule_address(rng, a[int(rng.integers(2))], r.src_bits)
    return r.validate()


def random_filters(frames, recs, seed=SEED, count=240):
    """`count` filters of 1..16 rules, inverted or not. The first rule of
    filter i carries the i-th valid `tests` combination, so every combination
    nexg_select_batch accepts occurs; the other rules lean to few tests, so
    that filters select something."""
    rng = np.random.default_rng(seed + 4)
    combos = _valid_test_combinations()
    assert len(combos) == 200 and count >= len(combos)
    good = [i for i in range(len(frames)) if (int(recs["flags"][i]) >> abi.STATUS_SHIFT) & 7 == 0]
    out = []
    for i in range(count):
        rules = []
        for k in range(int(rng.choice([1, 1, 2, 3, 5, 16]))):
            t = combos[i % len(combos)] if k == 0 else combos[int(rng.integers(len(combos)))]
            if k and rng.random() < 0.6:  # keep at most two of its tests
                bits = [b for b in (1 << np.arange(9)) if t & b]
                t = int(sum(rng.permutation(bits)[:2])) if bits else 0
            j = good[int(rng.integers(len(good)))]
            rules.append(random_rule(rng, t, frames[j], recs[j]))
        out.append(Filter(rules, invert=bool(rng.random() < 0.25)).validate())
    return out


# ---- flow ----------------------------------------------------------------------------------------

def flow_frames(seed=SEED):
    """(frames, count of the leading mutated ones): the select fuzz corpus, the
    flow hand corpus, and the ties of the symmetric compare."""
    frames, mutated = select_frames(seed)
    ties = []
    for l4 in ("tcp", "udp"):
        for a, b in ((ff.A4, ff.A4), (ff.A6, ff.A6), (sf.X6, sf.X6)):
            ties += [ff._tuple(l4, a, b, 9, 7, "").frame, ff._tuple(l4, a, b, 7, 9, "").frame,  # ports either way round
                     ff._tuple(l4, a, b, 5, 5, "").frame]                                        # everything equal
        # addresses that differ only in their last word, the ports deciding the other way
        ties += [ff._tuple(l4, Y6, sf.X6, 9, 7, "").frame, ff._tuple(l4, sf.X6, Y6, 7, 9, "").frame,
                 ff._tuple(l4, Y6, sf.X6, 7, 9, "").frame, ff._tuple(l4, sf.X6, Y6, 9, 7, "").frame]
        ties += [ff._tuple(l4, "10.0.0.1", "10.0.0.0", 7, 9, "").frame, ff._tuple(l4, "10.0.0.0", "10.0.0.1", 9, 7, "").frame]
    own = [x.frame for x in ff.own_corpus()]
    return frames + own + ties, mutated


def flow_keys(seed=SEED):
    """(name, 40-byte key or None for the default): the default key, 6 random
    keys, all-zero, all-ones, and single-bit keys at bits 0, 31, 32, 287, 319."""
    rng = np.random.default_rng(seed + 5)
    keys = [("default", None)] + [(f"random {i}", _rnd(rng, 40)) for i in range(6)]
    keys += [("zero", bytes(40)), ("ones", b"\xff" * 40)]
    for bit in (0, 31, 32, 287, 319):
        keys.append((f"bit {bit}", (1 << (319 - bit)).to_bytes(40, "big")))
    return keys


def key_bytes(key):
    return DEFAULT_KEY if key is None else key


def partition_hashes(count, buckets, seed=SEED):
    """name -> `count` u32 hashes: random, all equal, all in one residue class
    of `buckets`, sorted ascending and descending."""
    rng = np.random.default_rng(seed + 6 + count + buckets)
    rand = rng.integers(0, 1 << 32, count, dtype=np.uint64).astype(np.uint32)
    residue = (rng.integers(0, (1 << 32) // buckets - 1, count, dtype=np.uint64) * buckets + (buckets - 1) % buckets)
    return {"random": rand, "all equal": np.full(count, 0x9E3779B9, np.uint32), "one residue": residue.astype(np.uint32),
            "ascending": np.sort(rand), "descending": np.sort(rand)[::-1].copy()}


BUCKETS = (1, 2, 3, 7, 255, 256)


# ---- the corpora, built once -------------------------------------------------------------------

class Corpora:
    """Frames and the oracle's records of each corpus, with the corpus
    conditions asserted."""

    def __init__(self, oracle):
        self.dns = dns_frames()
        self.dns_recs = oracle_records(oracle, self.dns, DNS_PARSE_FLAGS)
        self.dns_stats = check_dns(self.dns, self.dns_recs)
        self.tun = tunnel_frames()
        self.tun_recs = oracle_records(oracle, self.tun, DNS_PARSE_FLAGS)
        self.tun_stats = check_decap(self.tun, self.tun_recs)
        self.sel, self.sel_mutated = select_frames()
        self.sel_recs = oracle_records(oracle, self.sel, SELECT_PARSE_FLAGS)
        check_status_ok(self.sel_recs, self.sel_mutated)
        self.filters = random_filters(self.sel, self.sel_recs)
        self.flow, self.flow_mutated = flow_frames()
        self.flow_recs = oracle_records(oracle, self.flow, SELECT_PARSE_FLAGS)
        check_status_ok(self.flow_recs, self.flow_mutated)
        self.keys = flow_keys()

    @functools.lru_cache(maxsize=None)
    def verdicts(self, k):
        """The independent reference's (selected, rule) arrays of filter k on the select corpus."""
        v = [ref.filter_verdict(f, r, len(f), self.filters[k]) for f, r in zip(self.sel, self.sel_recs)]
        return np.array([x[0] for x in v], bool), np.array([x[1] for x in v], np.uint8)

    def gpu_filters(self):
        """The 32 filters of the GPU sweep: the first, going through the list
        in steps of three, that select between 1 % and 99 % of the corpus."""
        n, picks = len(self.sel), []
        for k in (k for start in range(3) for k in range(start, len(self.filters), 3)):
            if len(picks) < 32 and 0.01 * n <= self.verdicts(k)[0].sum() <= 0.99 * n:
                picks.append(k)
        assert len(picks) == 32, len(picks)
        return picks


_CORPORA = None


def corpora(oracle) -> Corpora:
    global _CORPORA
    if _CORPORA is None:
        _CORPORA = Corpora(oracle)
    return _CORPORA


def batch_indices(n, seed, count=5083):
    """`count` corpus indices in shuffled order: a corpus smaller than the
    batch is repeated (whole permutations, so every frame occurs), a larger one
    subsampled. 5083 frames are 19 whole 256-frame tiles and 4 whole
    1024-frame partition tiles, each followed by a ragged one."""
    rng = np.random.default_rng(seed)
    idx = np.concatenate([rng.permutation(n) for _ in range(count // n + 1)])
    return idx[:count]
