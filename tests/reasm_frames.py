"""The reassembly corpus (a corpus module, not a test): tables of input frames
for nexg_reasm_plan / nexg_reasm_frames and nex_amd.reassemble.reassemble_host.

Trains are made by nex_amd.fragment.fragment_frame of tests/fragment_frames.py's
frames at mtu 68, 576 and 1500, each datagram given an identification of its
own (the corpus frames all share one), then put in order, reversed, shuffled
and interleaved; hand-made trains cover every way a datagram is incomplete.
cases() gives [(name, classes, frames)]; the module asserts that every class
the pass has to meet is there."""
import functools
import random

from nex_amd.fragment import fragment_frame
from tests import fragment_frames as ff

MTUS = (68, 576, 1500)

#: two sources whose (source, DST_C, 17) keys have one Toeplitz hash under the
#: default key: the hash is linear over GF(2), the difference of the two lies in
#: the kernel of the map from the 32 source bits' key windows (found once by
#: elimination; tests/test_reasm_host.py checks the equality)
SRC_A = bytes([10, 1, 2, 3])
SRC_B = bytes([0xE7, 0x19, 0x2E, 0xDE])
DST_C = bytes([10, 9, 8, 7])

CLASSES = ("in order", "reversed", "shuffled", "interleaved", "same addresses, other id", "same id, other addresses",
           "missing first", "missing middle", "missing last", "duplicate", "overlap", "gap of 8", "last with MF",
           "middle without MF", "data not a multiple of 8", "zero data", "head options, parts none", "exactly 65535",
           "65536", "8183 pieces", "input was a fragment", "trailing bytes", "bad extent", "VLAN", "IPv6", "ARP",
           "collision", "whole")


def retag(frame: bytes, ident=None, src=None, dst=None) -> bytes:
    """An IPv4 frame with another identification / addresses and its header checksum put right."""
    hl = 4 * (frame[14] & 15)
    h = bytearray(frame[14:14 + hl])
    if ident is not None:
        h[4:6] = ff.be(ident)
    if src is not None:
        h[12:16] = src
    if dst is not None:
        h[16:20] = dst
    h[10:12] = b"\0\0"
    h[10:12] = ff.be(ff.rfc1071(bytes(h)))
    return frame[:14] + bytes(h) + frame[14 + hl:]


def piece(ident, fo, mf, d, opts=b"", trailer=0, flags=0, src=None, dst=None, seed=0):
    """A hand-made fragment: offset fo (8-byte units), MF `mf`, d data bytes."""
    f = ff.ipv4(d, opts, word=flags | (0x2000 if mf else 0) | fo, ident=ident, trailer=trailer, seed=seed + fo)
    return retag(f, src=src, dst=dst) if src or dst else f


def train(frame: bytes, mtu: int, ident: int):
    return fragment_frame(retag(frame, ident), mtu)[0]


def is_ipv4(f):
    return f is not None and len(f) >= 34 and f[12:14] == b"\x08\x00" and f[14] >> 4 == 4 and f[14] & 15 >= 5


@functools.lru_cache(maxsize=None)
def sources():
    """The corpus frames of tests/fragment_frames.py that are whole IPv4 datagrams with DF clear and no bytes past
    the total length: what fragment -> reassemble gives back byte for byte."""
    out = []
    for name, f in ff.corpus():
        if not is_ipv4(f):
            continue
        hl, tl, word = 4 * (f[14] & 15), int.from_bytes(f[16:18], "big"), int.from_bytes(f[20:22], "big")
        if 14 + hl <= len(f) and hl <= tl and len(f) == 14 + tl and word & 0x7FFF == 0:
            out.append((name, f))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cases():
    rng = random.Random(20260721)
    ident = iter(range(0x1000, 0xFFFF))
    c = []

    def add(name, classes, frames):
        c.append((name, frozenset(classes), tuple(frames)))

    # ---- trains of the fragment corpus, every order
    small = [(n, f) for n, f in sources() if len(f) < 4200]
    for mtu in MTUS:
        for how in ("in order", "reversed", "shuffled"):
            table = []
            for name, f in small:
                t = list(train(f, mtu, next(ident)))
                if how == "reversed":
                    t.reverse()
                elif how == "shuffled":
                    rng.shuffle(t)
                table += t
            add(f"mtu {mtu}: every train {how}", {how, "whole"}, table)
        # two and three datagrams interleaved piece by piece
        table = []
        for k in range(0, len(small) - 2, 3):
            ts = [list(train(small[k + j][1], mtu, next(ident))) for j in range(2 + k % 2)]
            while any(ts):
                for t in ts:
                    if t:
                        table.append(t.pop(rng.randrange(len(t))))
        add(f"mtu {mtu}: datagrams interleaved", {"interleaved", "shuffled"}, table)
    big = [(n, f) for n, f in sources() if len(f) >= 4200]
    table = []
    for k, (name, f) in enumerate(big):
        t = list(train(f, MTUS[k % 3] if len(f) < 60000 else 1500, next(ident)))
        rng.shuffle(t)
        table += t
    add("the long frames, shuffled", {"shuffled"}, table)
    # ---- keys
    f = ff.ipv4(1200, seed=3)
    a, b = train(f, 576, 0x7001), train(f, 576, 0x7002)
    add("same addresses, other id", {"same addresses, other id"}, [a[0], b[1], b[0], a[2], b[2], a[1]])
    g = retag(ff.ipv4(1300, seed=4), src=bytes([192, 0, 2, 1]), dst=bytes([198, 51, 100, 2]))
    a, b = train(f, 576, 0x7003), train(g, 576, 0x7003)
    add("same id, other addresses", {"same id, other addresses"}, [a[0], b[0], b[2], a[2], a[1], b[1]])
    # ---- incomplete, one way each; a complete neighbour stands in front and behind
    def broken(name, cls, pieces):
        ok1, ok2 = train(ff.ipv4(700, seed=8), 576, next(ident)), train(ff.ipv4(900, ff.RA, seed=9), 576, next(ident))
        add(name, {cls}, [ok1[1], *pieces, ok1[0], ok2[0], ok2[1]])

    t = train(ff.ipv4(3000, seed=10), 576, 0x7200)
    assert len(t) == 6
    broken("missing first", "missing first", t[1:])
    broken("missing middle", "missing middle", t[:2] + t[3:])
    broken("missing last", "missing last", t[:-1])
    broken("duplicate piece", "duplicate", t + [t[2]])
    i = 0x7300
    broken("overlap", "overlap", [piece(i, 0, 1, 64), piece(i, 7, 1, 64), piece(i, 15, 0, 30)])
    broken("gap of 8 bytes", "gap of 8", [piece(i + 1, 0, 1, 64), piece(i + 1, 9, 0, 30)])
    broken("last piece with MF", "last with MF", [piece(i + 2, 0, 1, 64), piece(i + 2, 8, 1, 30)])
    broken("middle piece without MF", "middle without MF", [piece(i + 3, 0, 1, 64), piece(i + 3, 8, 0, 64), piece(i + 3, 16, 0, 30)])
    broken("a non-last piece of 60 bytes", "data not a multiple of 8", [piece(i + 4, 0, 1, 60), piece(i + 4, 8, 0, 30)])
    broken("a non-last piece of 4 bytes", "data not a multiple of 8", [piece(i + 5, 0, 1, 4), piece(i + 5, 1, 0, 30)])
    broken("zero data in the middle", "zero data", [piece(i + 6, 0, 1, 64), piece(i + 6, 8, 1, 0), piece(i + 6, 8, 0, 30)])
    broken("zero data last", "zero data", [piece(i + 7, 0, 1, 64), piece(i + 7, 8, 0, 0)])
    broken("a lone first piece", "missing last", [piece(i + 8, 0, 1, 64)])
    broken("a lone last piece", "missing first", [piece(i + 9, 8, 0, 64)])
    # ---- complete, the odd ones
    add("head with 40 option bytes, parts with none", {"head options, parts none"},
        [piece(i + 10, 8, 1, 16), piece(i + 10, 0, 1, 64, ff.OPTIONS["forty bytes"], flags=0x8000), piece(i + 10, 10, 0, 3)])
    add("DF and the reserved bit stay", {"head options, parts none"},
        [piece(i + 11, 0, 1, 8, flags=0xC000), piece(i + 11, 1, 0, 1, ff.RA)])
    add("pieces with bytes behind the total length", {"trailing bytes"},
        [piece(i + 12, 0, 1, 24, trailer=5), piece(i + 12, 3, 1, 8, trailer=1), piece(i + 12, 4, 0, 7, trailer=9)])
    add("hl + D is 65535", {"exactly 65535"}, [piece(i + 13, 4095, 0, 32755), piece(i + 13, 0, 1, 32760)])
    add("hl + D is 65536", {"65536"}, [piece(i + 14, 4095, 0, 32756), piece(i + 14, 0, 1, 32760)])
    add("hl 60 + D is 65535 / 65536", {"exactly 65535", "65536"},
        [piece(i + 15, 0, 1, 32760, ff.OPTIONS["forty bytes"]), piece(i + 15, 4095, 0, 32715),
         piece(i + 16, 0, 1, 32760, ff.OPTIONS["forty bytes"]), piece(i + 16, 4095, 0, 32716)])
    add("a part's 40 option bytes do not count: 20 + D is 65535", {"exactly 65535"},
        [piece(i + 17, 0, 1, 32760), piece(i + 17, 4095, 0, 32755, ff.OPTIONS["forty bytes"])])
    u, t = train(ff.ipv4(1200, proto=17, seed=12), 576, i + 18), train(ff.ipv4(1250, proto=6, seed=13), 576, i + 18)
    add("same id and addresses, other protocol", {"same id, other addresses"}, [u[0], t[1], t[0], u[2], t[2], u[1]])
    # ---- a train whose input was itself a fragment: never complete
    for name, f in ff.corpus():
        if name in ("fragment: first of a train (MF)", "fragment: middle (MF, offset 370)", "fragment: last (offset 740)"):
            t = list(train(f, 576, next(ident)))
            rng.shuffle(t)
            add(f"pieces of a {name}", {"input was a fragment"}, t)
    # ---- not fragments
    by_name = dict(ff.corpus())
    add("pass-through", {"bad extent", "VLAN", "IPv6", "ARP", "whole"},
        [by_name["VLAN-tagged IPv4"], None, by_name["IPv6 over 1500"], by_name["ARP"], by_name["IPv4 of 34 bytes"],
         by_name["Ethernet padding, fits"], by_name["empty"], by_name["13 bytes"], None, by_name["not IPv4: IHL 4"],
         by_name["not IPv4: total length one past the frame"], by_name["DF set"]])
    # ---- the pinned collision: one hash, one identification, two sources
    a = train(retag(ff.ipv4(1200, seed=5), src=SRC_A, dst=DST_C), 576, 0x7400)
    b = train(retag(ff.ipv4(1300, seed=6), src=SRC_B, dst=DST_C), 576, 0x7400)
    other = train(retag(ff.ipv4(1000, seed=7), src=SRC_A, dst=DST_C), 576, 0x7401)  # one hash, another id: not mixed
    add("collision", {"collision"}, [a[0], b[1], other[1], a[2], b[0], a[1], other[0], b[2]])
    return tuple(c)


@functools.lru_cache(maxsize=None)
def long_train():
    """The 8183 pieces of a 65535-byte frame with 40 option bytes at mtu 68, in order."""
    t = train(dict(ff.corpus())["65535 bytes, hl 60"], 68, 0x7500)
    assert len(t) == 8183
    return tuple(t)


def all_classes():
    have = set().union(*(cls for _, cls, _ in cases()))
    if len(long_train()) == 8183:  # kept out of cases(): its tests place it themselves
        have.add("8183 pieces")
    return have


@functools.lru_cache(maxsize=None)
def table(limit=4200):
    """Every case whose frames are all under `limit` bytes, one after the other: (frames, case of each frame)."""
    frames, owner = [], []
    for k, (_, _, fs) in enumerate(cases()):
        if all(f is None or len(f) < limit for f in fs):
            frames += fs
            owner += [k] * len(fs)
    return tuple(frames), tuple(owner)


assert all_classes() >= set(CLASSES), set(CLASSES) - all_classes()
