"""Differential sweep of the frame builders (nex_amd/csrc/nexg_build.hip and
nexg_build_probe.hip): the case grid, the launcher predicates restated as DISPATCH_CLASSES, the inputs
with planted extreme and solved-checksum rows, the oracle's expected bytes and
the whole-buffer comparer. tests/test_builder_sweep.py checks the grid, the
corpus and the comparer on the CPU; tests/test_gpu_builder_sweep.py runs it.

A Case names its optional per-frame arrays by the row they fill:

  src         udp4: src_ip, arp: sender_ip (absent: the batch default)
  src_shared  udp6 / tcp / icmp: src_ip holds one address (absent: one per frame)
  p0, p1      source / destination port; icmp: identifier / sequence
  ip_id, seq, ack, src_mac, dst_mac
              (arp: src_mac = sender_mac, dst_mac = eth_dst), target_mac (arp)
  multicast   ndp_ns: eth_dst_multicast (not an array)

udp4_tuples always carries src, p0, p1 and ip_id in its records. Whatever
the launchers of those two files test is restated here, so DISPATCH_CLASSES must be
updated whenever a launcher's predicates change."""
import ctypes
import itertools
from collections import namedtuple

import numpy as np

from nex_amd import abi, probes

Case = namedtuple("Case", "builder family form arrays payload_len pay_shift options out_stride out_shift count")

BUILDERS = ("udp4", "udp4_tuples", "udp6", "tcp", "icmp", "arp", "ndp_ns")
COUNTS = (1, 255, 256, 257, 513)  # the tile is 256 frames; 513 = two whole tiles and a one-frame tail
GUARD = 64                        # untouched bytes required before out and after out + count * out_stride
FILL = 0xA5                       # the output buffer's fill before the call
PAY_FILL = 0xEE                   # the payload buffer's bytes around the payload
K_SMALL_PAY = 64                  # kSmallPay
OPTIONAL = {
    "udp4": ("src", "p0", "p1", "ip_id", "src_mac", "dst_mac"),
    "udp4_tuples": (),
    "udp6": ("src_shared", "p0", "p1", "src_mac", "dst_mac"),
    "tcp": ("src_shared", "ip_id", "src_mac", "dst_mac", "p0", "p1", "seq", "ack"),
    "icmp": ("src_shared", "ip_id", "src_mac", "dst_mac", "p0", "p1"),
    "arp": ("src", "src_mac", "target_mac", "dst_mac"),
    "ndp_ns": ("src_mac", "dst_mac", "multicast"),
}
TCP_OPTIONS = (b"", b"\x01", probes.TCP_PING_OPTS, bytes(range(1, 41)))


def opt_padded(c):
    return (len(c.options) + 3) // 4 * 4


def frame_len(c):
    l3 = 20 if c.family == 4 else 40
    return {"udp4": 42 + c.payload_len, "udp4_tuples": 42 + c.payload_len, "udp6": 62 + c.payload_len,
            "tcp": 14 + l3 + 20 + opt_padded(c) + c.payload_len, "icmp": 14 + l3 + 8 + c.payload_len,
            "arp": 42, "ndp_ns": 86}[c.builder]


def is_probe(builder, arrays):
    """The probe form: one source, a destination per frame and nothing else per frame."""
    if builder == "udp4":
        return not arrays
    return builder in ("udp6", "tcp", "icmp") and tuple(arrays) == ("src_shared",)


def mk(builder, family=4, arrays=(), payload_len=0, pay_shift=0, options=b"", stride=None, out_shift=0, count=257):
    arrays = tuple(a for a in OPTIONAL[builder] if a in arrays)
    c = Case(builder, family, "probe" if is_probe(builder, arrays) else "general", arrays, payload_len, pay_shift,
             options, 0, out_shift, count)
    return c._replace(out_stride=frame_len(c) if stride is None else stride)


# ---------------------------------------------------------------- dispatch classes

def _aligned(c):
    return c.out_shift % 16 == 0


def _staged(c):  # `staged` of every launcher: out_stride <= kBuildMaxStride and out 16-B aligned
    return c.out_stride <= 128 and _aligned(c)


def _band2(c):  # MAXS of the launchers with a 64-B and a 128-B tile (0: direct global writes)
    return 0 if not _staged(c) else 64 if c.out_stride <= 64 else 128


def _band3(c):  # launch_l4_form: MAXS 64 / 80 / 128 / 0
    return 0 if not _staged(c) else 64 if c.out_stride <= 64 else 80 if c.out_stride <= 80 else 128


def _probe_launch_ok(c):  # probe_launch_ok(flen, period, pay_len, out)
    return c.out_stride <= 128 and frame_len(c) <= c.out_stride and c.payload_len <= K_SMALL_PAY and _aligned(c)


def _lane_launch_ok(c):  # lane_launch_ok(flen, period, pay_len, out): kLaneMaxP = 96
    return c.out_stride <= 96 and frame_len(c) <= c.out_stride and c.payload_len <= K_SMALL_PAY and _aligned(c)


def _kch(c):  # launch_probe: kch from need = ceil(P / 16)
    need = (c.out_stride + 15) // 16
    return 3 if need <= 3 else need if need <= 6 else 8


def _lane_instance(c):  # launch_lane: p48 / p68 (p48 only for ICMP over IPv4), else the generic instance
    p = c.out_stride
    if c.builder == "icmp" and c.family == 4 and 44 <= p <= 48:
        return "48,44"
    return "68,64" if 64 <= p <= 68 else "96"


def _udp4_form(c):  # launch_build_udp4: `full`, `probe`, else the general kernel
    a = set(c.arrays)
    if {"src", "p0", "p1", "ip_id"} <= a and not a & {"src_mac", "dst_mac"}:
        return "full"
    return "probe" if not a else "general"


def _udp6_template(c):  # launch_build_udp6's `probe` and try_probe_udp6
    return c.builder == "udp6" and c.form == "probe" and _probe_launch_ok(c)


def _l4_template(c):  # try_probe_l4 in the product library: tcp_ping probe batches take k_build_probe
    return c.builder == "tcp" and c.form == "probe" and _probe_launch_ok(c)


def _l4_lane(c):  # try_probe_l4 in the product library: ICMP over IPv4 probe batches take k_build_lane
    return c.builder == "icmp" and c.form == "probe" and c.family == 4 and _lane_launch_ok(c)


def _classes():
    out = []

    def add(name, gap, pred):
        out.append((name, gap, pred))

    def gap(maxs):  # the staged tiles zero [L, out_stride); the direct kernels leave it as it was
        return 0 if maxs else FILL

    # launch_build_udp4: FULL / PROBE only in the 64-B tile
    for form in ("full", "probe", "general"):
        add(f"k_build_udp4<64,{form}>", 0,
            lambda c, form=form: c.builder == "udp4" and _band2(c) == 64 and _udp4_form(c) == form)
    for m in (128, 0):
        add(f"k_build_udp4<{m}>", gap(m), lambda c, m=m: c.builder == "udp4" and _band2(c) == m)
    # launch_build_udp4_tuples
    for m in (64, 128, 0):
        add(f"k_build_udp4<{m},aos>", gap(m), lambda c, m=m: c.builder == "udp4_tuples" and _band2(c) == m)
    # launch_build_udp6: try_probe_udp6 -> launch_probe(dw = 4), else the per-lane kernel by stride band
    for k in (4, 5, 6, 8):  # 62 B and up: kch 3 is out of reach
        add(f"k_build_probe<4,{k},4> udp6", 0, lambda c, k=k: _udp6_template(c) and _kch(c) == k)
    for m in (64, 128, 0):
        add(f"k_build_udp6<{m}>", gap(m),
            lambda c, m=m: c.builder == "udp6" and not _udp6_template(c) and _band2(c) == m)
    # launch_l4_fam / try_probe_l4 / launch_probe / launch_lane / launch_l4_form
    for fam, dw in ((4, 1), (6, 4)):
        for k in (4, 5, 6, 8):
            if fam == 6 and k == 4:
                continue  # a TCP/IPv6 frame is 74 B at least
            add(f"k_build_probe<{dw},{k},4> tcp{fam}", 0,
                lambda c, fam=fam, k=k: _l4_template(c) and c.family == fam and _kch(c) == k)
    for inst in ("48,44", "68,64", "96"):
        add(f"k_build_lane<4,icmp,{inst}>", 0, lambda c, inst=inst: _l4_lane(c) and _lane_instance(c) == inst)
    for kind in ("tcp", "icmp"):
        for fam in (4, 6):
            for form in ("probe", "general"):
                for m in (64, 80, 128, 0):
                    if not _l4_form_reachable(kind, fam, form, m):
                        continue
                    add(f"k_build_l4<{fam},{kind},{m},{form}>", gap(m),
                        lambda c, kind=kind, fam=fam, form=form, m=m: c.builder == kind and c.family == fam and
                        c.form == form and not _l4_template(c) and not _l4_lane(c) and _band3(c) == m)
    # launch_build_arp, launch_build_ndp_ns
    for m in (64, 128, 0):
        add(f"k_build_arp<{m}>", gap(m), lambda c, m=m: c.builder == "arp" and _band2(c) == m)
    for m in (128, 0):
        add(f"k_build_ndp_ns<{m}>", gap(m), lambda c, m=m: c.builder == "ndp_ns" and _staged(c) == bool(m))
    return out


def _l4_form_reachable(kind, fam, form, m):
    """Instances of k_build_l4 that launch_l4_form can reach in the product
    library: the API refuses out_stride < frame length, and a probe batch that
    the template or the per-lane template kernel takes never gets here."""
    fmin = 14 + (20 if fam == 4 else 40) + (20 if kind == "tcp" else 8)
    if m and m < fmin:
        return False  # TCP/IPv6 (74 B) has no 64-B tile
    if form == "general" or m == 0:
        return True
    if kind == "tcp":  # staged probe: aligned and <= 128 B, so only a payload past kSmallPay brings it here
        return m == 128 and fmin + K_SMALL_PAY + 1 <= 128
    if fam == 4:       # ICMP/IPv4: k_build_lane takes periods up to 96 B
        return m == 128
    return True        # ICMP/IPv6 probe batches stay in k_build_l4


DISPATCH_CLASSES = _classes()


def classify(c):
    """(name, gap byte) of the one dispatch class that takes the case."""
    hits = [(n, g) for n, g, pred in DISPATCH_CLASSES if pred(c)]
    assert len(hits) == 1, (c, hits)
    return hits[0]


# ---------------------------------------------------------------- the grid

def max_payload(builder, family, options=b""):
    """The largest payload the entry accepts (the NEXG_ERANGE rules of nexg.h)."""
    if builder in ("udp4", "udp4_tuples"):
        return 65535 - 28
    if builder == "udp6":
        return 65535 - 8
    seg = 65535 - 20 if family == 4 else 65535
    return seg - (20 + (len(options) + 3) // 4 * 4 if builder == "tcp" else 8)


def pairwise(names):
    """Presence sets of `names` covering every pair of names in all four
    combinations: all, none, and each bit of a distinct code per name with its
    complement."""
    k = len(names)
    bits = max(1, (k - 1).bit_length())
    rows = [tuple(names), ()]
    for b in range(bits):
        on = tuple(n for i, n in enumerate(names) if (i >> b) & 1)
        rows += [on, tuple(n for n in names if n not in on)]
    return list(dict.fromkeys(rows))


def _forms(builder):
    """(probe form, a general form) of a builder, or its only form."""
    return {"udp4": [(), ("src", "p0", "p1", "ip_id"), ("src", "p0")], "udp4_tuples": [()],
            "udp6": [("src_shared",), ()], "tcp": [("src_shared",), ("p0",)], "icmp": [("src_shared",), ("p0",)],
            "arp": [()], "ndp_ns": [("multicast",)]}[builder]


def _families(builder):
    return (4, 6) if builder in ("tcp", "icmp") else (6,) if builder in ("udp6", "ndp_ns") else (4,)


def cases():
    """The covering set (deterministic): every dispatch class at every count
    and every out alignment that reaches it, the stride, payload-length,
    payload-shift and TCP-option edges, and the optional arrays pairwise."""
    out = []
    unal = itertools.cycle((1, 4, 8))
    for b in BUILDERS:
        for fam in _families(b):
            for arrays in _forms(b):
                base = mk(b, fam, arrays)
                L = frame_len(base)
                strides = {L, L + 1} | {s for s in (64, 65, 80, 81, 128, 129) if s >= L}
                if b == "icmp" and fam == 4 and base.form == "probe":  # k_build_lane's period windows
                    strides |= {s for s in (43, 44, 48, 49, 63, 64, 68, 69, 96, 97) if s >= L}
                if base.form == "probe" and b in ("tcp", "udp6"):     # k_build_probe: a period per kch
                    strides |= {s for s in (64, 72, 80, 96, 97, 112) if s >= L}
                for s in sorted(strides):
                    for n in COUNTS:
                        out.append(mk(b, fam, arrays, stride=s, count=n))
                    u = next(unal)
                    for n in (COUNTS if s == L else (257,)):
                        out.append(mk(b, fam, arrays, stride=s, out_shift=u, count=n))
                if b in ("arp", "ndp_ns"):
                    continue
                # staged probe batches past kSmallPay (k_build_l4<4,*,128,probe>) at every count
                if base.form == "probe" and b in ("tcp", "icmp") and fam == 4:
                    for n in COUNTS:
                        out.append(mk(b, fam, arrays, payload_len=65, count=n))
                # payload lengths, aligned and unaligned out
                for plen in (1, 2, 3, 4, 5, 61, 63, 64, 65, 66, 300, 515):
                    out.append(mk(b, fam, arrays, payload_len=plen))
                    out.append(mk(b, fam, arrays, payload_len=plen, out_shift=next(unal)))
                # payload address shifts on both sides of sh + n = 64, and inside k_build_lane's windows
                lens = [1, 3, 4, 61, 63, 64]
                if b == "icmp" and fam == 4 and base.form == "probe":
                    lens += [23, 26, 54]
                for sh in (1, 2, 3):
                    for plen in lens:
                        both = b in ("tcp", "icmp") or (b == "udp6" and base.form == "probe")
                        al = (0, next(unal)) if both else (0,) if (sh + plen) % 2 else (next(unal),)
                        for o in al:
                            out.append(mk(b, fam, arrays, payload_len=plen, pay_shift=sh, out_shift=o))
                if b == "icmp" and fam == 4 and base.form == "probe":
                    out += [mk(b, fam, arrays, payload_len=p) for p in (23, 26, 54)]
                if b == "tcp":
                    for opts in TCP_OPTIONS[1:]:
                        for plen in (0, 5):
                            out.append(mk(b, fam, arrays, payload_len=plen, options=opts))
                            out.append(mk(b, fam, arrays, payload_len=plen, options=opts, out_shift=next(unal)))
    # the largest payload each entry accepts, all 0xFF (payload_bytes), once per family for udp and tcp
    out += [mk("udp4", 4, (), payload_len=max_payload("udp4", 4)),
            mk("udp6", 6, (), payload_len=max_payload("udp6", 6)),
            mk("tcp", 4, ("p0",), payload_len=max_payload("tcp", 4)),
            mk("tcp", 6, ("src_shared",), payload_len=max_payload("tcp", 6))]
    # the optional arrays pairwise, in a staged and in a direct kernel
    for b in BUILDERS:
        for fam in _families(b):
            for arrays in pairwise(OPTIONAL[b]):
                for o in (0, next(unal)):
                    out.append(mk(b, fam, arrays, payload_len=0 if b in ("arp", "ndp_ns") else 7, out_shift=o))
    return list(dict.fromkeys(out))


# ---------------------------------------------------------------- inputs

_FIELDS16 = ("ip_id", "p0", "p1")
_FIELDS32 = ("seq", "ack")
_MACS = ("src_mac", "dst_mac", "target_mac")
_base_cache = {}


def _addr_bytes(c):
    return 4 if c.family == 4 or c.builder in ("udp4", "udp4_tuples", "arp") else 16


def _base_rows(c):
    """Random rows with the extreme rows planted at lanes 0, 63, 64 and 255 of
    every tile and at the last frame."""
    key = (c.builder, c.family, c.count)
    if key in _base_cache:
        return _base_cache[key]
    rng = np.random.default_rng([BUILDERS.index(c.builder), c.family, c.count])
    n, w = c.count, _addr_bytes(c)
    rows = {"src": rng.integers(0, 256, (n, w), dtype=np.uint8), "dst": rng.integers(0, 256, (n, w), dtype=np.uint8)}
    for f in _MACS:
        rows[f] = rng.integers(0, 256, (n, 6), dtype=np.uint8)
    for f in _FIELDS16:
        rows[f] = rng.integers(0, 1 << 16, n, dtype=np.uint32).astype(np.uint16)
    for f in _FIELDS32:
        rows[f] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)

    def plant(i, ones_addr, ones_fields):
        rows["src"][i] = rows["dst"][i] = 0xFF if ones_addr else 0
        for f in _FIELDS16:
            rows[f][i] = 0xFFFF if ones_fields else 0
        for f in _FIELDS32:
            rows[f][i] = 0xFFFFFFFF if ones_fields else 0

    for t0 in range(0, n, 256):
        for lane, (a, f) in ((0, (1, 1)), (63, (0, 0)), (64, (1, 0)), (255, (0, 1))):
            if t0 + lane < n:
                plant(t0 + lane, a, f)
    if (n - 1) % 256 not in (0, 63, 64, 255):
        plant(n - 1, 0, 0)
    _base_cache[key] = rows
    return rows


def payload_bytes(c, seed):
    if c.builder in ("arp", "ndp_ns") or c.payload_len == 0:
        return b""
    if c.payload_len == max_payload(c.builder, c.family, c.options):
        return b"\xff" * c.payload_len
    return np.random.default_rng([seed, 7]).integers(0, 256, c.payload_len, dtype=np.uint8).tobytes()


def _per_frame(c, f):
    if c.builder == "udp4_tuples":
        return f in ("src", "p0", "p1", "ip_id")
    if f == "src" and c.builder in ("udp6", "tcp", "icmp"):
        return "src_shared" not in c.arrays
    if f == "src" and c.builder == "ndp_ns":
        return True
    return f in c.arrays


L4_CK = "l4"
IP_CK = "ip"
SOLVE_PLAN = ((L4_CK, 0x0000), (IP_CK, 0x0000), (L4_CK, 0x0001), (IP_CK, 0xFFFF), (L4_CK, 0xFFFF), (IP_CK, 0x0001))


def checksum_offset(c, which):
    """Byte offset of the IPv4 header or the L4 checksum in the frame, or None."""
    if which == IP_CK:
        return 24 if (c.family == 4 and c.builder != "arp") else None
    l3 = 14 + (20 if c.family == 4 else 40)
    return {"udp4": 40, "udp4_tuples": 40, "udp6": 60, "tcp": l3 + 16, "icmp": l3 + 2, "arp": None,
            "ndp_ns": 56}[c.builder]


def _be16(frames, row, off):
    return (int(frames[row, off]) << 8) | int(frames[row, off + 1])


def _operand(c, which):
    """(row key, multiplicity in the sum) of the free 16-bit operand: the low
    half of the destination address, or for ICMP over IPv4 (no pseudo-header)
    a per-frame sequence / identifier array."""
    if which == L4_CK and c.builder == "icmp" and c.family == 4:
        return ("p1", 1) if "p1" in c.arrays else ("p0", 1) if "p0" in c.arrays else (None, 0)
    return ("dst", 2 if which == L4_CK and c.builder == "ndp_ns" else 1)  # NDP: pseudo-header and target


def _get_op(rows, key, r):
    return (int(rows["dst"][r, -2]) << 8 | int(rows["dst"][r, -1])) if key == "dst" else int(rows[key][r])


def _set_op(rows, key, r, v):
    if key == "dst":
        rows["dst"][r, -2:] = (v >> 8, v & 0xFF)
    else:
        rows[key][r] = v


def solve_checksum(oracle, c, inp, row, which, target, frames=None):
    """Adjust the free operand of `row` so that the oracle's frame carries the
    checksum `target` (0x0000 and 0xFFFF are the same residue: which of them
    the oracle emits is its to say). Ones'-complement arithmetic from the
    oracle's own output for the row; the caller re-checks against the oracle."""
    key, mult = _operand(c, which)
    off = checksum_offset(c, which)
    if key is None or off is None:
        return False
    frames = expected(oracle, c, inp, fresh=True) if frames is None else frames
    have = ~_be16(frames, row, off) & 0xFFFF          # the folded sum the oracle reached
    want = ~target & 0xFFFF
    step = (want - have) * pow(mult, -1, 0xFFFF)      # mod 0xFFFF (odd: 2 has an inverse)
    _set_op(inp["rows"], key, row, (_get_op(inp["rows"], key, row) + step) % 0xFFFF)
    return True


def inputs(c, seed, oracle=None):
    """Per-field numpy arrays (`rows`: every field per frame, the batch default
    repeated where the case has no array), the batch defaults and constants,
    the payload and the solved rows [(row, which, target)]."""
    if oracle is None:
        from oracle import oracle
    rng = np.random.default_rng([seed, 1])
    base, n, w = _base_rows(c), c.count, _addr_bytes(c)
    d = {"src": rng.integers(0, 256, w, dtype=np.uint8)}
    for f in _MACS:
        d[f] = rng.integers(0, 256, 6, dtype=np.uint8)
    for f in _FIELDS16:
        d[f] = int(rng.integers(0, 1 << 16))
    for f in _FIELDS32:
        d[f] = int(rng.integers(0, 1 << 32))
    const = {"ttl": int(rng.integers(0, 256)), "ip_flags": int(rng.integers(0, 8)), "tos": int(rng.integers(0, 256)),
             "flow_label": int(rng.integers(0, 1 << 32)), "window": int(rng.integers(0, 1 << 16)),
             "urg": int(rng.integers(0, 1 << 16)), "tcp_flags": int(rng.integers(0, 256)),
             "icmp_type": 8 if c.family == 4 else 128, "icmp_code": int(rng.integers(0, 256)),
             "arp_operation": 1 + seed % 2}
    if c.builder == "icmp" and c.family == 4 and c.payload_len == 0 and seed % 3 == 0:
        # an all-zero echo reply: the only message whose sum is 0 (checksum 0xFFFF)
        const["icmp_type"] = const["icmp_code"] = d["p0"] = d["p1"] = 0
    rows = {}
    for f in ("src",) + _MACS + _FIELDS16 + _FIELDS32:
        if _per_frame(c, f):
            rows[f] = base[f].copy()
        else:
            rows[f] = np.broadcast_to(np.asarray(d[f], base[f].dtype), base[f].shape).copy()
    rows["dst"] = base["dst"].copy()
    inp = {"rows": rows, "defaults": d, "const": const, "payload": payload_bytes(c, seed), "solved": []}
    if c.builder == "icmp" and c.family == 4 and not {"p0", "p1"} & set(c.arrays) and seed % 2 == 0 \
            and const["icmp_type"]:
        # one checksum for the whole batch: solve it through the batch's sequence number
        target = (0x0000, 0x0001, 0xFFFF)[seed // 2 % 3]
        f0 = expected(oracle, c, inp, fresh=True)
        have, want = ~_be16(f0, 0, checksum_offset(c, L4_CK)) & 0xFFFF, ~target & 0xFFFF
        d["p1"] = (d["p1"] + want - have) % 0xFFFF
        rows["p1"][:] = d["p1"]
        inp["solved"].append((0, L4_CK, target))
    # solved rows at lane 0 and the last lane of the ragged tile first, then their neighbours
    cand = list(dict.fromkeys(r for r in (0, n - 1, 1, n - 2, 2, n - 3) if 0 <= r < n))
    plan = [SOLVE_PLAN[(seed + k) % len(SOLVE_PLAN)] for k in range(len(SOLVE_PLAN))]
    frames = expected(oracle, c, inp, fresh=True)
    for which, target in plan:
        if cand and solve_checksum(oracle, c, inp, cand[0], which, target, frames):
            inp["solved"].append((cand.pop(0), which, target))
    got = expected(oracle, c, inp, fresh=True)
    for row, which, target in inp["solved"]:
        ck = _be16(got, row, checksum_offset(c, which))
        assert ck == target or (target in (0, 0xFFFF) and ck in (0, 0xFFFF)), (c, row, which, hex(target), hex(ck))
    return inp


def expected(oracle, c, inp, fresh=False):
    """(count, L) uint8: every frame from the oracle's single-frame builders
    (oracle.build_rows_batch loops over them)."""
    if not fresh and "want" in inp:
        return inp["want"]
    r, k = dict(inp["rows"]), inp["const"]
    kind = "udp4" if c.builder == "udp4_tuples" else c.builder
    if c.builder == "ndp_ns" and "multicast" in c.arrays:  # examples/ndp.rs: 33:33 + the target's last four bytes
        r["dst_mac"] = np.concatenate([np.full((c.count, 2), 0x33, np.uint8), r["dst"][:, 12:16]], axis=1)
    if c.builder == "ndp_ns":
        k = dict(k, ip_flags=0)
    if c.builder in ("udp6", "ndp_ns", "arp") or c.family == 6:
        r["ip_id"] = None
    fam = 4 if _addr_bytes(c) == 4 else 6
    spec = oracle.ip_spec(fam, b"", b"", ttl=k["ttl"], ip_flags=k["ip_flags"], dscp_ecn=k["tos"],
                          flow_label=k["flow_label"])
    want = oracle.build_rows_batch(kind, spec, r, options=c.options, payload=inp["payload"], window=k["window"],
                                   urg=k["urg"], tcp_flags=k["tcp_flags"], icmp_type=k["icmp_type"],
                                   icmp_code=k["icmp_code"], arp_hw_type=1, arp_proto_type=0x0800,
                                   arp_operation=k["arp_operation"])
    assert want.shape == (c.count, frame_len(c)), (c, want.shape)
    if not fresh:
        inp["want"] = want
    return want


# ---------------------------------------------------------------- the comparer

def buffer_bytes(c):
    return GUARD + 16 + c.count * c.out_stride + GUARD


def layout(c, want, gap):
    """The whole buffer a correct build leaves: guards and slack FILL, the
    frames, the gaps `gap`."""
    buf = np.full(buffer_bytes(c), FILL, np.uint8)
    lo = GUARD + c.out_shift
    fr = buf[lo: lo + c.count * c.out_stride].reshape(c.count, c.out_stride)
    fr[:, :frame_len(c)] = want
    fr[:, frame_len(c):] = gap
    return buf


def compare(c, buf, want, cls=None):
    """Check the whole buffer after the call (FILL before it): every frame
    equals the oracle's, every gap [L, out_stride) is the byte the dispatch
    class leaves there (`cls`: (name, gap), default the product library's class
    for the case), and nothing outside [out, out + count * out_stride) changed."""
    name, gap = cls or classify(c)
    n, S, L = c.count, c.out_stride, frame_len(c)
    assert buf.shape == (buffer_bytes(c),) and buf.dtype == np.uint8
    lo = GUARD + c.out_shift
    fr = buf[lo: lo + n * S].reshape(n, S)

    def fail(what, i=None, off=None):
        msg = [f"{what}", f"case {c}", f"dispatch class {name}"]
        if i is not None:
            msg += [f"frame {i} (lane {i % 256}), first differing byte offset {off}",
                    f"got  {fr[i, :max(L, off + 1)].tobytes().hex()}", f"want {want[i].tobytes().hex()}"]
        raise AssertionError("\n".join(msg))

    bad = np.nonzero((fr[:, :L] != want).any(axis=1))[0]
    if bad.size:
        i = int(bad[0])
        fail(f"{bad.size} frames differ from the oracle's", i, int(np.nonzero(fr[i, :L] != want[i])[0][0]))
    if S > L:
        bad = np.nonzero((fr[:, L:] != gap).any(axis=1))[0]
        if bad.size:
            i = int(bad[0])
            fail(f"gap bytes of {bad.size} frames are not {gap:#04x}", i, L + int(np.nonzero(fr[i, L:] != gap)[0][0]))
    if (buf[:lo] != FILL).any():
        fail(f"bytes before out written: buffer offset {int(np.nonzero(buf[:lo] != FILL)[0][0])} (out at {lo})")
    if (buf[lo + n * S:] != FILL).any():
        fail(f"bytes after out + count * out_stride written: "
             f"{int(np.nonzero(buf[lo + n * S:] != FILL)[0][0])} B past the end")


# ---------------------------------------------------------------- running a case on the GPU

def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _u32_values(addr):
    """(n, 4) network-order bytes as the BE u32 values nexg_udp4_build takes."""
    return np.ascontiguousarray(addr).view(">u4").reshape(-1).astype(np.uint32)


def wrapper_ok(c):
    """Whether the Engine wrapper can express the case: it has no per-frame MAC
    arrays, and it tells a shared source from a one-frame batch by the count."""
    if {"src_mac", "dst_mac"} & set(c.arrays) and c.builder != "arp":
        return False
    return not (c.count == 1 and "src_shared" in c.arrays)


def launch(engine, c, inp, raw=None):
    """Build the case into a FILL-ed buffer with guards; returns (device
    buffer, out view). Through the Engine wrapper where it can express the
    case, else through the raw library entry."""
    import torch
    r, d, k = inp["rows"], inp["defaults"], inp["const"]
    n, S = c.count, c.out_stride
    buf = torch.full((buffer_bytes(c),), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    out = buf[GUARD + c.out_shift: GUARD + c.out_shift + n * S]
    pay = None
    if inp["payload"]:
        pbuf = torch.full((c.pay_shift + c.payload_len + 32,), PAY_FILL, dtype=torch.uint8, device="cuda")
        assert pbuf.data_ptr() % 16 == 0
        pay = pbuf[c.pay_shift: c.pay_shift + c.payload_len]
        pay.copy_(torch.frombuffer(bytearray(inp["payload"]), dtype=torch.uint8))
    t = {}  # device arrays of the per-frame fields the case passes
    for f in ("src",) + _MACS + _FIELDS16 + _FIELDS32:
        if _per_frame(c, f):
            t[f] = _dev(_u32_values(r[f]) if f == "src" and c.builder in ("udp4", "udp4_tuples") else r[f])
    udp4 = c.builder in ("udp4", "udp4_tuples")
    t["dst"] = _dev(_u32_values(r["dst"]) if udp4 else r["dst"])
    if "src" not in t and c.builder in ("udp6", "tcp", "icmp"):
        t["src"] = _dev(d["src"])  # the one shared source
    smac, dmac = bytes(d["src_mac"]), bytes(d["dst_mac"])
    use_raw = (not wrapper_ok(c)) if raw is None else raw
    g = t.get
    if not use_raw:
        if c.builder == "udp4":
            engine.build_udp4(g("src"), t["dst"], g("p0"), g("p1"), g("ip_id"), d["p0"], d["p1"], d["ip_id"], smac, dmac,
                              k["ttl"], k["ip_flags"], k["tos"], pay, S, out,
                              def_src_ip=int.from_bytes(bytes(d["src"]), "big"))
        elif c.builder == "udp4_tuples":
            tup = engine.pack_udp4_tuples(t["src"], t["dst"], t["p0"], t["p1"], t["ip_id"])
            engine.build_udp4_tuples(tup, smac, dmac, k["ttl"], k["ip_flags"], k["tos"], pay, S, out)
        elif c.builder == "udp6":
            engine.build_udp6(t["src"], t["dst"], g("p0"), g("p1"), d["p0"], d["p1"], smac, dmac, k["ttl"], k["tos"],
                              k["flow_label"], pay, S, out)
        elif c.builder == "tcp":
            engine.build_tcp(c.family, t["src"], t["dst"], g("p0"), g("p1"), g("seq"), g("ack"), d["p0"], d["p1"],
                             d["seq"], d["ack"], k["tcp_flags"], k["window"], k["urg"], c.options, pay, g("ip_id"),
                             d["ip_id"], smac, dmac, k["ttl"], k["ip_flags"], k["tos"], k["flow_label"], S, out)
        elif c.builder == "icmp":
            engine.build_icmp_echo(c.family, t["src"], t["dst"], g("p0"), g("p1"), d["p0"], d["p1"], k["icmp_type"],
                                   k["icmp_code"], pay, g("ip_id"), d["ip_id"], smac, dmac, k["ttl"], k["ip_flags"],
                                   k["tos"], k["flow_label"], S, out)
        elif c.builder == "arp":
            engine.build_arp(t["dst"], g("src"), bytes(d["src"]), g("src_mac"), smac, g("target_mac"),
                             bytes(d["target_mac"]), g("dst_mac"), dmac, operation=k["arp_operation"], out_stride=S,
                             out=out)
        else:
            engine.build_ndp_ns(t["src"], t["dst"], smac, None if "multicast" in c.arrays else dmac, k["ttl"], k["tos"],
                                k["flow_label"], S, out)
        return buf, out
    ptr = lambda f: None if f not in t else t[f].data_ptr()
    args = (ctypes.c_void_p(out.data_ptr()), S, engine._stream(None))

    def ip_build(ip):
        ip.src_ip, ip.dst_ip, ip.ip_id = t["src"].data_ptr(), t["dst"].data_ptr(), ptr("ip_id")
        ip.src_mac, ip.dst_mac = ptr("src_mac"), ptr("dst_mac")
        ip.family, ip.flow_label, ip.def_ip_id = c.family, k["flow_label"], d["ip_id"]
        ip.def_src_mac[:], ip.def_dst_mac[:] = list(smac), list(dmac)
        ip.ttl, ip.ip_flags, ip.tos, ip.src_shared = k["ttl"], k["ip_flags"], k["tos"], int("src_shared" in c.arrays)

    if udp4:
        p = abi.Udp4Build()
        if c.builder == "udp4":
            p.src_ip, p.dst_ip, p.src_port, p.dst_port, p.ip_id = ptr("src"), t["dst"].data_ptr(), ptr("p0"), ptr("p1"), \
                ptr("ip_id")
            p.src_mac, p.dst_mac = ptr("src_mac"), ptr("dst_mac")
            p.def_src_port, p.def_dst_port, p.def_ip_id = d["p0"], d["p1"], d["ip_id"]
            p.def_src_ip = int.from_bytes(bytes(d["src"]), "big")
        p.payload, p.payload_len = None if pay is None else pay.data_ptr(), c.payload_len
        p.def_src_mac[:], p.def_dst_mac[:] = list(smac), list(dmac)
        p.ttl, p.ip_flags, p.dscp_ecn, p.count = k["ttl"], k["ip_flags"], k["tos"], n
        if c.builder == "udp4":
            rc = engine.lib.nexg_build_udp4_batch(engine.ctx, ctypes.byref(p), *args)
        else:
            tup = engine.pack_udp4_tuples(t["src"], t["dst"], t["p0"], t["p1"], t["ip_id"])
            rc = engine.lib.nexg_build_udp4_tuples(engine.ctx, ctypes.byref(p), ctypes.c_void_p(tup.data_ptr()), *args)
    elif c.builder == "udp6":
        p = abi.Udp6Build()
        p.src_ip, p.dst_ip, p.src_port, p.dst_port = t["src"].data_ptr(), t["dst"].data_ptr(), ptr("p0"), ptr("p1")
        p.src_mac, p.dst_mac = ptr("src_mac"), ptr("dst_mac")
        p.payload, p.payload_len = None if pay is None else pay.data_ptr(), c.payload_len
        p.flow_label, p.def_src_port, p.def_dst_port = k["flow_label"], d["p0"], d["p1"]
        p.def_src_mac[:], p.def_dst_mac[:] = list(smac), list(dmac)
        p.hop_limit, p.traffic_class, p.src_shared, p.count = k["ttl"], k["tos"], int("src_shared" in c.arrays), n
        rc = engine.lib.nexg_build_udp6_batch(engine.ctx, ctypes.byref(p), *args)
    elif c.builder == "tcp":
        p = abi.TcpBuild()
        ip_build(p.ip)
        p.src_port, p.dst_port, p.seq, p.ack = ptr("p0"), ptr("p1"), ptr("seq"), ptr("ack")
        p.payload, p.payload_len = None if pay is None else pay.data_ptr(), c.payload_len
        p.def_seq, p.def_ack, p.def_src_port, p.def_dst_port = d["seq"], d["ack"], d["p0"], d["p1"]
        p.window, p.urgent_ptr, p.flags, p.options_len = k["window"], k["urg"], k["tcp_flags"], len(c.options)
        p.options[:len(c.options)] = list(c.options)
        p.count = n
        rc = engine.lib.nexg_build_tcp_batch(engine.ctx, ctypes.byref(p), *args)
    elif c.builder == "icmp":
        p = abi.IcmpEchoBuild()
        ip_build(p.ip)
        p.identifier, p.sequence = ptr("p0"), ptr("p1")
        p.payload, p.payload_len = None if pay is None else pay.data_ptr(), c.payload_len
        p.def_identifier, p.def_sequence, p.icmp_type, p.icmp_code = d["p0"], d["p1"], k["icmp_type"], k["icmp_code"]
        p.count = n
        rc = engine.lib.nexg_build_icmp_echo_batch(engine.ctx, ctypes.byref(p), *args)
    elif c.builder == "arp":
        p = abi.ArpBuild()
        p.target_ip, p.sender_ip, p.sender_mac = t["dst"].data_ptr(), ptr("src"), ptr("src_mac")
        p.target_mac, p.eth_dst = ptr("target_mac"), ptr("dst_mac")
        p.def_sender_ip[:], p.def_sender_mac[:] = list(bytes(d["src"])), list(smac)
        p.def_target_mac[:], p.def_eth_dst[:] = list(bytes(d["target_mac"])), list(dmac)
        p.hardware_type, p.protocol_type, p.operation = 1, 0x0800, k["arp_operation"]
        p.hw_addr_len, p.proto_addr_len, p.count = 6, 4, n
        rc = engine.lib.nexg_build_arp_batch(engine.ctx, ctypes.byref(p), *args)
    else:
        p = abi.NdpNsBuild()
        ip_build(p.ip)
        p.ip.ip_flags = 0
        p.eth_dst_multicast, p.count = int("multicast" in c.arrays), n
        rc = engine.lib.nexg_build_ndp_ns_batch(engine.ctx, ctypes.byref(p), *args)
    engine._check(rc)
    torch.cuda.synchronize()  # the arrays of `t` stay alive until the kernel has read them
    return buf, out


def run(engine, c, inp, raw=None):
    """The whole host buffer after the build."""
    import torch
    buf, _ = launch(engine, c, inp, raw)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


# ---------------------------------------------------------------- forms that must agree, knob classes

def equivalents(c):
    """Cases that must give frame-for-frame the bytes of `c` on the inputs of
    `c` (whose rows hold the batch default wherever `c` has no array): the
    general form with the source repeated per frame, the SoA form of a tuples
    build, and a per-frame array of the batch default."""
    out = []
    if c.form == "probe" and c.builder != "udp4":
        out.append(c._replace(arrays=(), form="general"))
    if c.form == "probe" and c.builder == "udp4":
        out.append(c._replace(arrays=("src",), form="general"))
    if c.builder == "udp4_tuples":
        out.append(c._replace(builder="udp4", arrays=("src", "p0", "p1", "ip_id")))
    if c.form == "general" and c.builder not in ("udp4_tuples", "arp", "ndp_ns"):
        extra = next((f for f in ("p1", "ip_id", "p0") if f in OPTIONAL[c.builder] and f not in c.arrays), None)
        if extra:
            out.append(c._replace(arrays=tuple(a for a in OPTIONAL[c.builder] if a in c.arrays + (extra,))))
    return out


KNOB_SETTINGS = ("NEXG_PROBE_ICMP=1", "NEXG_PROBE_ICMP=2", "NEXG_PROBE_LANE_TCP=1", "NEXG_PROBE_WAVES=1")


def knob_class(c, setting):
    """(name, gap) of the instance the measurement library picks for a probe
    case under one setting of try_probe_l4's / launch_probe's overrides, or
    None where the setting does not bear on the case."""
    if c.form != "probe":
        return None
    dw = 1 if c.family == 4 else 4
    rest = lambda: (f"k_build_l4<{c.family},{c.builder},{_band3(c)},probe>", 0 if _band3(c) else FILL)
    if setting == "NEXG_PROBE_ICMP=1" and c.builder == "icmp":  # the template kernel for both families
        return (f"k_build_probe<{dw},{_kch(c)},4> icmp{c.family}", 0) if _probe_launch_ok(c) else rest()
    if setting == "NEXG_PROBE_ICMP=2" and c.builder == "icmp":  # the per-lane k_build_l4 for both families
        return rest()
    if setting == "NEXG_PROBE_LANE_TCP=1" and c.builder == "tcp":  # k_build_lane when the payload is empty
        if c.payload_len == 0 and _lane_launch_ok(c):
            return (f"k_build_lane<{c.family},tcp,{'68,64' if 64 <= c.out_stride <= 68 else '96'}>", 0)
        return (f"k_build_probe<{dw},{_kch(c)},4> tcp{c.family}", 0) if _probe_launch_ok(c) else rest()
    if setting == "NEXG_PROBE_WAVES=1" and c.builder in ("tcp", "udp6"):  # the one-wave template kernel
        if _probe_launch_ok(c):
            return (f"k_build_probe<{dw},{_kch(c)},1> {'udp6' if c.builder == 'udp6' else 'tcp%d' % c.family}", 0)
        return classify(c)
    return None
