"""The corpus of the header rewrite (nexg_rewrite_batch) and an independent
reference, shared by tests/test_rewrite_host.py, test_rewrite_core.py,
test_cpp_rewrite.py and the GPU tests.

rewrite_ref does not import nex_amd.rewrite: it takes its views from the
oracle's fix-up report of the untouched frame (which views recompute_checksum
was chained through), edits the bytes, and in RECOMPUTE mode passes them
through oracle.recompute_frame with `which` = the dirty set; in INCREMENTAL
mode it applies RFC 1624 eqn. 3 to the words that differ in kind, read from the
frame before and after the edit. Actions are plain Act tuples here; to_set()
turns them into the package's builders."""
import functools
from collections import namedtuple

import numpy as np

from nex_amd import abi
from tests import helpers
from tests.fixup_sweep import PROTO, _icmp, _l4, _rnd

BOTH = abi.FIX_IP | abi.FIX_L4
PAYLOADS = (0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 1471)
RAW_OFFSETS = (0, 1, 13)
MAX_FRAME = 65535
ADDR = abi.SET_IP_SRC | abi.SET_IP_DST
PORTS = abi.SET_SRC_PORT | abi.SET_DST_PORT

Act = namedtuple("Act", "name sets family ttl tos tos_mask src_port dst_port eth_dst eth_src src dst",
                 defaults=(0, 0, 0, 0, 0, 0, 0, bytes(6), bytes(6), bytes(16), bytes(16)))

S4, D4 = bytes([192, 0, 2, 1]).ljust(16, b"\0"), bytes([198, 51, 100, 7]).ljust(16, b"\0")
S6, D6 = bytes.fromhex("20010db8000000000000000000000001"), bytes.fromhex("20010db800ff00000000ffff00000007")
M1, M2 = bytes.fromhex("02a0b0c0d0e1"), bytes.fromhex("02a0b0c0d0e2")
# what helpers._eth / _ipv4 / _ipv6 / _udp put into a frame
OLD_DST_MAC, OLD_SRC_MAC = bytes(range(1, 7)), bytes(range(7, 13))
OLD_S4, OLD_D4 = bytes([10, 1, 2, 3]).ljust(16, b"\0"), bytes([10, 4, 5, 6]).ljust(16, b"\0")
OLD_S6, OLD_D6 = bytes(range(16)), bytes(range(16, 32))

NAT44 = Act("nat44 + ports + dec_ttl", ADDR | PORTS | abi.DEC_TTL, 4, ttl=1, src_port=40000, dst_port=443, src=S4, dst=D4)
ACTIONS = (
    Act("eth_dst", abi.SET_ETH_DST, eth_dst=M1),
    Act("eth_src", abi.SET_ETH_SRC, eth_src=M2),
    Act("ip_src 4", abi.SET_IP_SRC, 4, src=S4),
    Act("ip_dst 4", abi.SET_IP_DST, 4, dst=D4),
    Act("ip_src 6", abi.SET_IP_SRC, 6, src=S6),
    Act("ip_dst 6", abi.SET_IP_DST, 6, dst=D6),
    Act("src_port", abi.SET_SRC_PORT, src_port=0xC001),
    Act("dst_port", abi.SET_DST_PORT, dst_port=0xFFFF),
    Act("set_ttl 7", abi.SET_TTL, ttl=7),
    Act("dec_ttl 3", abi.DEC_TTL, ttl=3),
    Act("tos 0xb8", abi.SET_TOS, tos=0xB8, tos_mask=0xFF),
    NAT44,
    Act("nat66 + ports", ADDR | PORTS, 6, src_port=1, dst_port=65535, src=S6, dst=D6),
    Act("router: macs + dec_ttl 1", abi.SET_ETH_DST | abi.SET_ETH_SRC | abi.DEC_TTL, ttl=1, eth_dst=M1, eth_src=M2),
    Act("dscp (mask 0xfc)", abi.SET_TOS, tos=0x28 << 2 & 0xFC, tos_mask=0xFC),
    Act("ecn (mask 0x03)", abi.SET_TOS, tos=0x3, tos_mask=0x03),
    Act("set_ttl 0", abi.SET_TTL, ttl=0),
    Act("set_ttl 255", abi.SET_TTL, ttl=255),
    Act("dec_ttl past 0", abi.DEC_TTL, ttl=200),
    Act("same values 4", abi.SET_ETH_DST | abi.SET_ETH_SRC | ADDR | PORTS | abi.SET_TTL, 4, ttl=64, src_port=0x04D2,
        dst_port=0x0035, eth_dst=OLD_DST_MAC, eth_src=OLD_SRC_MAC, src=OLD_S4, dst=OLD_D4),
    Act("same values 6", ADDR | PORTS | abi.SET_TTL, 6, ttl=64, src_port=0x1234, dst_port=0x0050, src=OLD_S6, dst=OLD_D6),
    Act("all-ones / all-zero addresses 4", ADDR, 4, src=b"\xff" * 4 + bytes(12), dst=bytes(16)),
    Act("all-zero / all-ones addresses 6", ADDR, 6, src=bytes(16), dst=b"\xff" * 16),
    Act("everything 4", abi.SET_ALL & ~abi.DEC_TTL, 4, ttl=9, tos=0x55, tos_mask=0x7F, src_port=7, dst_port=9, eth_dst=M1,
        eth_src=M2, src=S4, dst=D4),
    Act("everything 6", abi.SET_ALL & ~abi.SET_TTL, 6, ttl=2, tos=0xA0, tos_mask=0xF0, src_port=0x8000, dst_port=0x7FFF,
        eth_dst=M2, eth_src=M1, src=S6, dst=D6),
    Act("leave it"),
)
NAMES = tuple(a.name for a in ACTIONS)
assert len(set(NAMES)) == len(NAMES)


def action_chunks():
    """ACTIONS in sets of at most 16 (NEXG_REWRITE_MAX_ACTIONS): [(first index, actions)]."""
    return [(i, ACTIONS[i:i + 16]) for i in range(0, len(ACTIONS), 16)]


def to_action(a):
    from nex_amd.rewrite import Action
    return Action(sets=a.sets, family=a.family, ttl=a.ttl, tos=a.tos, tos_mask=a.tos_mask, src_port=a.src_port,
                  dst_port=a.dst_port, eth_dst=a.eth_dst, eth_src=a.eth_src, src=a.src, dst=a.dst)


def to_set(acts, incremental=False):
    from nex_amd.rewrite import ActionSet
    return ActionSet([to_action(a) for a in acts], incremental=incremental)


# ---------------------------------------------------------------- frames

def _v4(seg, proto, ihl=5, total=None, flags_frag=0x4000, ttl=64):
    ip = bytearray(helpers._ipv4(seg, proto, ihl=ihl, opts=bytes([1]) * (4 * ihl - 20), total=total,
                                 flags_frag=flags_frag))
    ip[8] = ttl
    ip[10:12] = b"\xba\xd2"  # stored header checksum: garbage
    return helpers._eth(bytes(ip))


def _v6(seg, nh):
    return helpers._eth(helpers._ipv6(seg, nh, plen=min(len(seg), 0xFFFF)), 0x86DD)


def _set16(frame, at, v):
    return frame[:at] + v.to_bytes(2, "big") + frame[at + 2:]


def garbage_frames(rng):
    """The frames as built: every stored checksum is garbage."""
    out = []
    for n in PAYLOADS:
        pay = _rnd(rng, n)
        for ihl in (5, 6, 15):
            for kind in ("udp", "tcp", "icmp"):
                out.append(_v4(_l4(kind, pay), PROTO[kind], ihl=ihl))
        out.append(_v4(_l4("tcp", pay, 15), 6))
        out.append(_v6(_l4("udp", pay), 17))
        out.append(_v6(_l4("tcp", pay, 5), 6))
        out.append(_v6(_l4("tcp", pay, 15), 6))
        out.append(_v6(_icmp(pay, 128), 58))
        out.append(_v4(pay, 50))  # no L4 view
    pay = _rnd(rng, 40)
    # one byte short of each view
    for cut in (13, 33, 41, 53, 61):
        for kind in ("udp", "tcp", "icmp"):
            out.append(_v4(_l4(kind, pay), PROTO[kind])[:cut])
    for cut in (13, 53, 61, 73):
        for seg, nh in ((_l4("udp", pay), 17), (_l4("tcp", pay), 6), (_icmp(pay, 128), 58)):
            out.append(_v6(seg, nh)[:cut])
    for i, kind in enumerate(("udp", "tcp", "icmp")):
        out.append(_v4(_l4(kind, pay), PROTO[kind], total=0))                # total_length 0
        out.append(_v4(_l4(kind, pay), PROTO[kind]) + _rnd(rng, 1 + 3 * i))  # trailing Ethernet padding
        out.append(_v4(_l4(kind, pay), PROTO[kind], ttl=1 + i))              # TTLs a DEC_TTL 3 takes to 0
    out += [_v4(helpers._udp(pay, length=0), 17), _v6(helpers._udp(pay, length=0), 17)]  # UDP length 0
    # first, middle and last IPv4 fragments: the later ones carry payload bytes where an L4 header would be
    for kind in ("udp", "tcp"):
        for ff in (0x2000, 0x2000 | 185, 370):
            out.append(_v4(_l4(kind, pay), PROTO[kind], flags_frag=ff))
    # stored UDP checksum 0 (IPv6: just one more garbage value)
    out += [_set16(_v4(helpers._udp(pay), 17), 34 + 6, 0), _set16(_v6(helpers._udp(pay), 17), 54 + 6, 0)]
    # stored checksums 0xFFFF
    out += [_set16(_set16(_v4(helpers._udp(pay), 17), 24, 0xFFFF), 40, 0xFFFF), _set16(_v6(_l4("tcp", pay), 6), 70, 0xFFFF)]
    out += helpers.vlan_frames()
    out += [helpers._eth(bytes(range(28)), 0x0806), helpers._eth(pay, 0x88B5), helpers._eth(b"", 0x0800), b"",
            bytes(12) + b"\x08"]
    return out


def _fix(oracle, frame, flags=0, ip_offset=0):
    return oracle.recompute_frame(frame, BOTH, flags, ip_offset)[0]


def planted_frames(oracle, rng):
    """Frames whose IPv4 header and L4 checksums come out 0x0000 and 0x0001
    AFTER the NAT44 action, solved as fixup_sweep._solve solves: a word no
    action touches (the IP id; the first payload word) takes up the difference."""
    out = []
    for target in (0x0000, 0x0001):
        for kind in ("udp", "tcp"):
            hdr = {"udp": 8, "tcp": 20}[kind]
            f = _v4(_l4(kind, _rnd(rng, 2 + int(rng.integers(0, 40)))), PROTO[kind])
            for word, field_name in ((14 + 4, "ip_csum"), (34 + hdr, "l4_csum")):
                _, row = rewrite_ref(f, NAT44, 0)
                have = ~int(row[REWRITTEN.index(field_name)]) & 0xFFFF
                w = (int.from_bytes(f[word:word + 2], "big") + (~target & 0xFFFF) - have) % 0xFFFF
                f = _set16(f, word, w)
                _, row = rewrite_ref(f, NAT44, 0)
                assert row[REWRITTEN.index(field_name)] == target, (kind, field_name, target, row)
            out.append(f)
    return out


Corpus = namedtuple("Corpus", "fixed garbage udp4_zero planted")
# fixed[i] / garbage[i]: the same frame with the checksums the oracle fixed / as built; udp4_zero: indices whose
# fixed form is UDP over IPv4 with the checksum field put back to 0 ("none"); planted: indices of planted_frames


@functools.lru_cache(maxsize=None)
def corpus():
    from oracle import oracle
    rng = np.random.default_rng(1624)
    garbage = garbage_frames(rng)
    first = len(garbage)
    garbage += planted_frames(oracle, rng)
    planted = tuple(range(first, len(garbage)))
    zero_at = {i for i, f in enumerate(garbage)
               if len(f) >= 42 and f[12:14] == b"\x08\x00" and f[23] == 17 and f[14] == 0x45 and f[40:42] == b"\0\0"}
    assert len(zero_at) == 1
    garbage.append(_v4(helpers._udp(_rnd(rng, MAX_FRAME - 14 - 20 - 8)), 17))  # the 65535-B frame
    fixed = []
    for i, f in enumerate(garbage):
        g = _fix(oracle, f)
        if i in zero_at:
            g = _set16(g, 40, 0)
        fixed.append(g)
    return Corpus(tuple(fixed), tuple(garbage), tuple(sorted(zero_at)), planted)


def small(frames, below=4096):
    return [i for i, f in enumerate(frames) if len(f) < below]


@functools.lru_cache(maxsize=None)
def raw_ip(k):
    """(fixed, garbage) IP packets of the corpus's IPv4 / IPv6 frames behind
    `k` junk bytes, for NEXG_PARSE_FROM_IP with ip_offset = k."""
    from oracle import oracle
    c = corpus()
    rng = np.random.default_rng(k)
    garbage = [_rnd(rng, k) + f[14:] for f in c.garbage if len(f) < 4096 and f[12:14] in (b"\x08\x00", b"\x86\xdd")]
    zero = {i for i, f in enumerate(garbage) if len(f) >= k + 28 and f[k] == 0x45 and f[k + 9] == 17 and f[k + 26:k + 28] == b"\0\0"}
    fixed = [_set16(g, k + 26, 0) if i in zero else g
             for i, g in enumerate(_fix(oracle, f, abi.PARSE_FROM_IP, k) for f in garbage)]
    return tuple(fixed), tuple(garbage)


# ---------------------------------------------------------------- the reference

REWRITTEN = ("applied", "fixed", "action", "ip_csum", "l4_csum")


def _fold(t):
    while t >> 16:
        t = (t & 0xFFFF) + (t >> 16)
    return t


def _w(f, i):
    return int.from_bytes(f[i:i + 2], "big")


def rewrite_ref(frame, act, a, incremental=False, flags=0, ip_offset=0):
    """(new bytes, (applied, fixed, action, ip_csum, l4_csum)) of one frame under Act `act`, number `a`."""
    from oracle import oracle
    if len(frame) > MAX_FRAME:
        return bytes(frame), (0, 0, a, 0, 0)
    old = bytes(frame)
    f = bytearray(old)
    from_ip = bool(flags & abi.PARSE_FROM_IP)
    # the views: what the oracle's chain of mutable views reaches on the untouched frame
    _, rep = oracle.recompute_frame(old, BOTH, flags, ip_offset)
    eth = not from_ip and len(f) >= 14
    L = ip_offset if from_ip else 14
    v4 = bool(int(rep["done"]) & abi.FIX_IP)
    if from_ip:
        v6 = len(f) - L >= 40 and f[L] >> 4 == 6 if L < len(f) else False
    else:
        v6 = eth and f[12:14] == b"\x86\xdd" and len(f) - 14 >= 40
    l4 = bool(int(rep["done"]) & abi.FIX_L4)
    proto, P = int(rep["proto"]), int(rep["l4_off"])
    if incremental and v4 and _w(f, L + 6) & 0x1FFF:
        l4 = False  # a later fragment holds no L4 header
    raw_proto = f[L + 9] if v4 else (f[L + 6] if v6 else 0)
    applied = 0
    ip_words, l4_words = [], []  # offsets of the 16-bit words the two checksums cover among the applied fields
    if eth:
        if act.sets & abi.SET_ETH_DST:
            f[0:6] = act.eth_dst
            applied |= abi.SET_ETH_DST
        if act.sets & abi.SET_ETH_SRC:
            f[6:12] = act.eth_src
            applied |= abi.SET_ETH_SRC
    if (v4 and act.family == 4) or (v6 and act.family == 6):
        n, at = (4, L + 12) if v4 else (16, L + 8)
        for bit, o, val in ((abi.SET_IP_SRC, at, act.src), (abi.SET_IP_DST, at + n, act.dst)):
            if act.sets & bit:
                f[o:o + n] = val[:n]
                applied |= bit
                ip_words += range(o, o + n, 2)
                if raw_proto != 1:
                    l4_words += range(o, o + n, 2)
    if (v4 or v6) and act.sets & (abi.SET_TTL | abi.DEC_TTL):
        at = L + 8 if v4 else L + 7
        f[at] = act.ttl if act.sets & abi.SET_TTL else max(f[at] - act.ttl, 0)
        applied |= act.sets & (abi.SET_TTL | abi.DEC_TTL)
        ip_words.append(L + 8)
    if (v4 or v6) and act.sets & abi.SET_TOS:
        if v4:
            f[L + 1] = (f[L + 1] & ~act.tos_mask & 255) | act.tos
        else:
            word = _w(f, L)
            tc = ((word >> 4 & 0xFF) & ~act.tos_mask & 255) | act.tos
            f[L:L + 2] = ((word & 0xF00F) | tc << 4).to_bytes(2, "big")
        applied |= abi.SET_TOS
        ip_words.append(L)
    if l4 and proto in (6, 17):
        if act.sets & abi.SET_SRC_PORT:
            f[P:P + 2] = act.src_port.to_bytes(2, "big")
            applied |= abi.SET_SRC_PORT
            l4_words.append(P)
        if act.sets & abi.SET_DST_PORT:
            f[P + 2:P + 4] = act.dst_port.to_bytes(2, "big")
            applied |= abi.SET_DST_PORT
            l4_words.append(P + 2)
    dirty = 0
    if v4 and applied & (ADDR | abi.SET_TTL | abi.DEC_TTL | abi.SET_TOS):
        dirty |= abi.FIX_IP
    if l4 and (applied & PORTS or (applied & ADDR and raw_proto != 1)):
        dirty |= abi.FIX_L4
    if not incremental:
        out, fx = oracle.recompute_frame(bytes(f), dirty, flags, ip_offset)
        assert int(fx["done"]) == dirty, (int(fx["done"]), dirty)
        return out, (applied, dirty, a, int(fx["ip_csum"]), int(fx["l4_csum"]))
    edited = bytes(f)
    fixed = ip_c = l4_c = 0
    if dirty & abi.FIX_IP:
        ip_c = ~_fold((~_w(old, L + 10) & 0xFFFF) + sum((~_w(old, o) & 0xFFFF) + _w(edited, o) for o in ip_words)) & 0xFFFF
        f[L + 10:L + 12] = ip_c.to_bytes(2, "big")
        fixed |= abi.FIX_IP
    if dirty & abi.FIX_L4:
        at = P + {17: 6, 6: 16}.get(proto, 2)
        hc = _w(old, at)
        if not (proto == 17 and v4 and hc == 0):
            l4_c = ~_fold((~hc & 0xFFFF) + sum((~_w(old, o) & 0xFFFF) + _w(edited, o) for o in l4_words)) & 0xFFFF
            f[at:at + 2] = l4_c.to_bytes(2, "big")
            fixed |= abi.FIX_L4
    return bytes(f), (applied, fixed, a, ip_c, l4_c)


_ref_cache = {}


def ref_all(frames, incremental, flags=0, ip_offset=0):
    """{action number: ([new frames], rows)} of `frames` (a tuple, kept) under
    every action of ACTIONS; computed once and never modified."""
    key = (id(frames), incremental, flags, ip_offset)
    if key not in _ref_cache:
        res = {}
        for a, act in enumerate(ACTIONS):
            got = [rewrite_ref(f, act, a % 16, incremental, flags, ip_offset) for f in frames]
            rows = np.array([r for _, r in got], abi.REWRITTEN_DTYPE) if got else np.zeros(0, abi.REWRITTEN_DTYPE)
            rows.setflags(write=False)
            res[a] = (tuple(b for b, _ in got), rows)
        _ref_cache[key] = (frames, res)
    return _ref_cache[key][1]


def row_tuple(r):
    return tuple(int(r[n]) for n in REWRITTEN)
