"""The far batch: one corpus of about 300 frames placed three times in a
device buffer of 2^32 + 2 MiB bytes, at byte 1, around 2^31 and around 2^32,
so that every pass runs with frame offsets at and above 2^31 and 2^32 while
only a few hundred KiB of the buffer are ever written.

Everything here is arithmetic on the host (no 4-GiB array is made): the
corpus, the three placements (what sits on each boundary), the four table
forms that describe the same bytes, the index maps from table row to frame,
and each pass's expectation per frame from its host contract.
tests/test_far_batch.py asserts the placements' anchors and the corpus's
strength; tests/test_gpu_far_batch.py runs the kernels.

The frames. corpus() takes frames of the existing corpora (DNS, tunnels,
select, flow with its collision pair, the hand cases of the match corpus, the
small rewrite frames, a TCP option sweep, planted fix-up frames); every frame
is under 2048 B but the select corpus's valid 65535-byte UDP/IPv4 frame. All
of them are parsed with NEXG_PARSE_VLAN | NEXG_PARSE_STRICT.

A placement's frame list is the corpus three times: cluster 0 from byte 1 in
corpus order, clusters 1 and 2 rotated so that the wanted frame sits where the
placement wants it relative to 2^31 and 2^32; inside a cluster the frames are
back to back.

    A   a short frame begins 9 bytes below the boundary
    B   one frame's last byte is boundary - 1, the next begins at the boundary
    C   the 65535-byte frame begins 30000 bytes below the boundary
    B1  B with cluster 2 one byte lower (the frame that begins at 2^32 in B
        begins at 0xFFFFFFFF): cut to 0xFFFFFFFF data bytes, the last frame
        kept ends on the last data byte, the largest batch without group bases

The table forms.

    1  u64 offsets + lengths: the 3 K corpus rows (2-GiB gaps between clusters)
    2  u32 offsets + lengths + bases: FrameBatch.with_offsets32() of form 1
    3  packed u64: dense, the zero bytes between clusters as filler frames of
       65535 zero bytes plus one shorter filler per gap (about 65.5k fillers,
       66.5k rows, 260 tiles)
    4  packed u32 + bases: with_offsets32() of form 3

Forms 1-2 also run on data views shorter than the buffer (Placement.rows_within):
the rows whose extent lies inside the view, a prefix of the table.

Frame ids. Far.frames is the corpus followed by the distinct filler frames
(Far.frames[K] is the 65535-byte one); Placement.ids / dense_ids give each
table row's id, and Expect holds one expectation per id."""
import functools
from collections import namedtuple

import numpy as np

from nex_amd import abi
from nex_amd.flow import FlowOption, flows_host
from nex_amd.frame import ParseOption
from nex_amd.match import NO_MATCH, Pattern, PatternSet, match_rows_host
from nex_amd.select import Filter, Rule

GIB2, GIB4 = 1 << 31, 1 << 32
BOUNDARIES = (GIB2, GIB4)
BUFFER_BYTES = GIB4 + (2 << 20)
NO_BASES_BYTES = 0xFFFFFFFF  # the largest data_bytes whose u32 table has no group bases
FILLER_LEN = 65535
PARSE_FLAGS = abi.PARSE_VLAN | abi.PARSE_STRICT
FIX_OPTION = ParseOption(unwrap_vlan=True)  # what the in-place passes parse with (they are lenient)
BOTH = abi.FIX_IP | abi.FIX_L4

#: where the wanted frame begins, relative to the boundary
SITUATIONS = {"A": -9, "B": 0, "C": -30000, "B1": 0}
PLACEMENTS = ("A", "B", "C")

# ---- what the passes are run with ----------------------------------------------------------

#: the first rule reads the IPv6 addresses from the frame's bytes (off + l3 + 8) for every frame
FILTER = Filter([Rule.net("2001:db8::/32", "src"), Rule.udp() & Rule.port(53), Rule.tcp(), Rule.udp(),
                 Rule.bad_checksum("l4")])
#: four patterns: the 65535-byte frames cost the host contract a step per byte and pattern. The last one's first
#: occurrence in the 65535-byte frame lies past byte 30000: past the boundary in C
PATTERNS = [Pattern(b"."), Pattern(b"xyz"), Pattern(b"hOsT:", nocase=True),
            Pattern(bytes([7, 8, 9, 10]), offset=(29990, 30300))]
MATCH_ANY, MATCH_NONE = 0b1011, 0b0100  # nexg_match_select: a dot, xyz or the far pattern, and no hOsT:
FLOW_OPTION = FlowOption()  # not symmetric: the collision pair collides in this direction
REWRITE_INDEX = list(range(16)) + [abi.ACTION_NONE, 16, 77]  # every action, and three ways to say "none"
NAT44 = 11  # rewrite_frames.ACTIONS[11]: addresses, ports and TTL, both checksums dirtied


def pattern_set(frame_mode):
    return PatternSet(PATTERNS, frame=frame_mode)


def action_set(incremental):
    from tests import rewrite_frames as rf
    first, acts = rf.action_chunks()[0]
    assert first == 0 and len(acts) == 16 and acts[NAT44] is rf.NAT44
    return rf.to_set(acts, incremental)


def rewrite_index(i):
    """The action number of frame id `i`: every third frame the NAT44 action."""
    return NAT44 if i % 3 == 0 else REWRITE_INDEX[i % len(REWRITE_INDEX)]


# ---- the corpus ------------------------------------------------------------------------------

Section = namedtuple("Section", "name first count")


@functools.lru_cache(maxsize=None)
def corpus():
    """(frames, sections): about 300 frames, one of them 65535 B."""
    from oracle import oracle
    from tests import dns_frames as df
    from tests import fixup_sweep as fx
    from tests import flow_frames as ff
    from tests import flow_group_frames as fg
    from tests import helpers
    from tests import match_frames as mf
    from tests import rewrite_frames as rf
    from tests import select_frames as sf
    from tests import tunnel_frames as tf
    rng = np.random.default_rng(4294967296 % 9973)
    parts = [("dns", [c.frame for c in df.cases()][:36]),
             ("tunnel", [c.frame for c in tf.cases()][:48]),
             ("select", [x.frame for x in sf.corpus()]),
             ("flow", [x.frame for x in ff.own_corpus()] + fg.collision_frames())]
    match = []
    for c in (mf.header_trap_cases()[0], *mf.shape_cases(), mf.nocase_cases()[0], mf.empty_cases()[0], mf.large_cases()[0]):
        match += [f for f in c.frames if len(f) < 2048]
    sweep = mf.sweep_case(5)
    match += [f for f, p in zip(sweep.frames, sweep.notes["planted"]) if p is None or p[0] == 16]
    parts.append(("match", match[:56]))
    rc = rf.corpus()
    small = rf.small(rc.garbage)
    parts.append(("rewrite", [rc.garbage[i] for i in small[::7]] + [rc.garbage[i] for i in rc.planted] +
                  [rc.fixed[i] for i in small[3::21]]))
    P = bytes(range(40))
    bases = ([helpers._eth(helpers._ipv4(helpers._tcp(P[:k]), 6)) for k in (0, 1, 7, 26)] +
             [helpers._eth(helpers._ipv6(helpers._tcp(P[:k]), 6), 0x86DD) for k in (0, 3, 40)])
    opts = helpers.tcp_option_sweep(oracle, rng, bases)
    parts.append(("tcp options", opts[:: len(opts) // 24][:24]))
    parts.append(("fix-up planted", [p.frame for p in fx.planted_frames(oracle, rng)][::2]))
    frames, sections = [], []
    for name, fr in parts:
        sections.append(Section(name, len(frames), len(fr)))
        frames += [bytes(f) for f in fr]
    big = [i for i, f in enumerate(frames) if len(f) >= 2048]
    assert len(big) == 1 and len(frames[big[0]]) == 65535
    assert 257 <= len(frames) <= 340, len(frames)  # over 256: no 256-frame group spans a whole cluster
    return tuple(frames), tuple(sections)


# ---- the placements --------------------------------------------------------------------------

class Placement:
    """One placement's tables on the host (int64 arrays)."""

    def __init__(self, name, K, lens, wanted, positions, bounds, filler_id):
        self.name, self.K, self.bounds = name, K, bounds
        self.wanted = wanted        # the corpus index of the wanted frame
        self.positions = positions  # its position inside clusters 1 and 2
        self.order = [np.arange(K)] + [(wanted - p + np.arange(K)) % K for p in positions]
        self.start = [1]
        for c in (1, 2):
            before = int(lens[self.order[c][: positions[c - 1]]].sum())
            self.start.append(bounds[c - 1] + SITUATIONS[name] - before)
        self.ids = np.concatenate(self.order)
        self.length = lens[self.ids]
        self.off = np.concatenate([self.start[c] + np.concatenate([[0], np.cumsum(lens[self.order[c]])[:-1]])
                                   for c in range(3)]).astype(np.int64)
        self.end = [self.start[c] + int(lens.sum()) for c in range(3)]
        assert self.end[0] <= self.start[1] and self.end[1] <= self.start[2] and self.end[2] <= BUFFER_BYTES
        #: boundary -> the row (forms 1-2) of the wanted frame
        self.row = {bounds[c - 1]: c * K + positions[c - 1] for c in (1, 2)}
        # the dense table: fillers between the clusters
        ids, dl, self.dense_row = [], [], np.zeros(3 * K, np.int64)
        n = 0
        for c in range(3):
            if c:
                full, rest = divmod(self.start[c] - self.end[c - 1], FILLER_LEN)
                ids.append(np.full(full, K, np.int64))
                dl.append(np.full(full, FILLER_LEN, np.int64))
                n += full
                if rest:
                    ids.append(np.array([filler_id(rest)], np.int64))
                    dl.append(np.array([rest], np.int64))
                    n += 1
            ids.append(self.order[c])
            dl.append(lens[self.order[c]])
            self.dense_row[c * K:(c + 1) * K] = n + np.arange(K)
            n += K
        self.dense_ids, self.dense_length = np.concatenate(ids), np.concatenate(dl)
        self.dense_off = np.concatenate([[1], 1 + np.cumsum(self.dense_length)]).astype(np.int64)
        assert (self.dense_off[self.dense_row] == self.off).all() and self.dense_off[-1] == self.end[2]
        self.dense_is_filler = self.dense_ids >= K

    def rows_within(self, data_bytes):
        """How many rows of forms 1-2 lie inside the first `data_bytes` bytes (a prefix: the table ascends)."""
        return int(np.searchsorted(self.off + self.length, data_bytes, side="right"))

    def cluster_bytes(self, frames, c):
        """Cluster c's bytes (uint8 array) of a list of per-id frames."""
        return np.frombuffer(b"".join(frames[i] for i in self.order[c]), np.uint8)

    def group_anchors(self, off, row, count):
        """What the anchors ask of the 256-frame group of `row` in a table with
        offsets `off`: neither the row nor the one before it (B's other
        boundary frame) is the group's first, the row is not its last, and
        (at 2^32) a later group of the table has its base at or above 2^32."""
        ok = row % 256 not in (0, 1, 255) and row + 1 < count
        later = (row // 256 + 1) * 256
        return ok, later < count and off[later] >= GIB4


def _search(build, c, K):
    """The first position from 24 on at which cluster c's wanted frame meets
    group_anchors in both the sparse and the dense table: two dozen frames of
    the cluster lie below the boundary, all the others at or above it."""
    for p in range(24, K - 2):
        pl = build(p)
        b = pl.bounds[c - 1]
        srow = pl.row[b]
        s_ok, s_later = pl.group_anchors(pl.off, srow, 3 * K)
        drow = int(pl.dense_row[srow])
        d_ok, d_later = pl.group_anchors(pl.dense_off, drow, len(pl.dense_ids))
        if s_ok and d_ok and (c == 1 or (s_later and d_later)):
            return p
    raise AssertionError(f"no position for cluster {c}")


class Far:
    """The corpus, the filler frames and the placements."""

    def __init__(self):
        self.corpus, self.sections = corpus()
        self.K = K = len(self.corpus)
        lens = np.array([len(f) for f in self.corpus], np.int64)
        self.fillers = [FILLER_LEN]  # distinct filler lengths: id K + j

        def filler_id(n):
            if n not in self.fillers:
                self.fillers.append(n)
            return K + self.fillers.index(n)

        # the two dozen frames below each boundary come from one large section (a small one would lose its strength)
        sec = next(s for s in self.sections if s.name == "rewrite")
        short = next(i for i in range(sec.first + 24, sec.first + sec.count)
                     if 42 <= lens[i] <= 64 and self.corpus[i][12:14] == b"\x08\x00")
        big = int(np.argmax(lens))
        dns = next(s for s in self.sections if s.name == "dns").first + 1
        assert lens[dns] > 0 and lens[dns - 1] > 0
        wanted = {"A": short, "B": dns, "C": big, "B1": dns}
        self.placements = {}
        for name in (*PLACEMENTS, "B1"):
            bounds = (GIB2, GIB4 - 1) if name == "B1" else BOUNDARIES

            def build(p1, p2, name=name, bounds=bounds):
                return Placement(name, K, lens, wanted[name], (p1, p2), bounds, filler_id)

            saved = list(self.fillers)
            p1 = _search(lambda p: build(p, K // 2), 1, K)
            p2 = _search(lambda p: build(p1, p), 2, K)
            self.fillers = saved  # the search's trial placements named fillers that no table keeps
            self.placements[name] = build(p1, p2)
        self.frames = list(self.corpus) + [bytes(n) for n in self.fillers]
        self.lengths = np.array([len(f) for f in self.frames], np.int64)
        for pl in self.placements.values():
            assert (self.lengths[pl.dense_ids] == pl.dense_length).all()


@functools.lru_cache(maxsize=None)
def far():
    return Far()


def table32(offsets, data_bytes, packed):
    """The NEXG_FRAMES_OFFSETS32 table FrameBatch.with_offsets32() builds from
    u64 offsets (count + 1 of a packed table, count beside lengths: the last
    slot repeats the last offset), and the u64 offsets it stands for."""
    o = np.asarray(offsets, np.uint64)
    if not packed:
        o = np.concatenate([o, o[-1:] if len(o) else np.zeros(1, np.uint64)])
    return abi.offsets32_table(o, data_bytes), o


# ---- the expectations, one per frame id ------------------------------------------------------

class Expect:
    """Each pass's host contract over Far.frames, computed on first use.
    Rows of a table are these arrays taken at the table's ids."""

    def __init__(self, f: Far):
        from oracle import oracle
        self.far, self.oracle = f, oracle
        self.frames, self.lengths, self.K = f.frames, f.lengths, f.K
        self.n = len(self.frames)

    @functools.cached_property
    def recs(self):
        return self.oracle.parse_frames(self.frames, PARSE_FLAGS)

    @functools.cached_property
    def desc(self):
        d = np.zeros(self.n, abi.DESC_DTYPE)
        for name in abi.DESC_DTYPE.names:
            d[name] = self.recs[name]
        return d

    def checksum(self, skipword):
        from tests.fixup_sweep import checksum_ref
        return np.array([checksum_ref(f, skipword) for f in self.frames], np.uint16)

    @functools.cached_property
    def fixup(self):
        """(fixed frames, nexg_fixup rows) of nexg_recompute_checksums_batch with FIX_OPTION."""
        out = [self.oracle.recompute_frame(f, BOTH, FIX_OPTION.flags(), 0) for f in self.frames]
        rows = np.zeros(self.n, abi.FIXUP_DTYPE)
        for i, (_, r) in enumerate(out):
            rows[i] = np.frombuffer(r.tobytes(), abi.FIXUP_DTYPE)[0]
        return [bytes(f) for f, _ in out], rows

    @functools.lru_cache(maxsize=None)
    def rewrite(self, incremental):
        """(rewritten frames, nexg_rewritten rows, index) of nexg_rewrite_batch with FIX_OPTION."""
        from nex_amd.rewrite import rewrite_host
        index = np.array([rewrite_index(i) for i in range(self.n)], np.uint8)
        index[self.K:] = NAT44  # the fillers: an action that finds nothing to set in a frame without an IP layer
        out, rows = rewrite_host(self.frames, action_set(incremental), index, FIX_OPTION)
        return out, rows, index

    @functools.cached_property
    def options(self):
        return np.array([self.oracle.decode_options(f, PARSE_FLAGS, 0) for f in self.frames], abi.OPTIONS_DTYPE)

    @functools.cached_property
    def tunnels(self):
        """(nexg_tunnel rows, inner offset inside the frame, inner length)."""
        from nex_amd.tunnel import decap_host
        from tests.tunnel_frames import tunnels_array
        out = [decap_host(f, r) for f, r in zip(self.frames, self.recs)]
        return (tunnels_array([t for t, _, _ in out]), np.array([o for _, o, _ in out], np.int64),
                np.array([n for _, _, n in out], np.uint32))

    @functools.cached_property
    def dns(self):
        """(nexg_dns rows with `first` 0, the entry rows of each frame)."""
        from nex_amd.dns import dns_frame_host
        from tests.dns_frames import entry_array, summary_array
        out = [dns_frame_host(f, r) for f, r in zip(self.frames, self.recs)]
        return summary_array([s for s, _ in out]), [entry_array(e) for _, e in out]

    @functools.cached_property
    def select(self):
        """(selected, rule) of FILTER per frame."""
        from nex_amd.select import match_host
        v = [match_host(f, r, len(f), FILTER) for f, r in zip(self.frames, self.recs)]
        return np.array([x[0] for x in v], bool), np.array([x[1] for x in v], np.uint8)

    @functools.cached_property
    def match_filler(self):
        """nexg_match_batch's row for a filler, from the 65535-byte zero frame
        in frame mode. Every pattern holds a nonzero byte, so no run of zero
        bytes contains one wherever its window lies: the shorter fillers and
        the payload mode (a part of the same zero bytes) have the same row."""
        pset = pattern_set(True)
        assert all(any(bytes(p.data)) for p in pset.patterns)
        K = self.K
        row = match_rows_host(self.frames[K: K + 1], None, self.lengths[K: K + 1], pset)[0]
        assert tuple(row)[:3] == NO_MATCH
        return row

    @functools.lru_cache(maxsize=None)
    def match(self, frame_mode):
        """nexg_match rows of pattern_set(frame_mode)."""
        K = self.K
        rows = np.zeros(self.n, abi.MATCH_DTYPE)
        rows[:K] = match_rows_host(self.frames[:K], self.recs, self.lengths, pattern_set(frame_mode))
        rows[K:] = self.match_filler
        return rows

    @functools.cached_property
    def flows(self):
        return flows_host(self.frames, self.recs, self.lengths, FLOW_OPTION)

    # -- what depends on the rows ---------------------------------------------------------------

    def dns_rows(self, ids):
        """(nexg_dns rows, tile_first, entry rows) of a table with these ids."""
        summaries, entries = self.dns
        n = len(ids)
        k = np.array([len(e) for e in entries], np.int64)[ids]
        before = np.concatenate([[0], np.cumsum(k)])
        tiles = (n + 255) // 256
        tile_first = np.array([before[256 * t] for t in range(tiles)] + [before[n]], np.uint64)
        want = summaries[ids].copy()
        want["first"] = before[:n] - tile_first[np.arange(n) >> 8].astype(np.int64)
        rows = [entries[i] for i in ids[k > 0]]
        return want, tile_first, np.concatenate(rows) if rows else np.zeros(0, abi.DNS_ENTRY_DTYPE)

    # -- the strength of the corpus -------------------------------------------------------------

    def strength(self, ids):
        """name -> how many of the frames `ids` meet the condition."""
        ids = np.asarray(ids)
        summaries, entries = self.dns
        tun = self.tunnels[0]
        sel, rule = self.select
        accepted = (tun["status"] == abi.FRAME_OK)
        out = {
            "dns summary without error, with entries":
                ((summaries["flags8"] & abi.DNS_CANDIDATE != 0) & (summaries["status"] == abi.FRAME_OK) &
                 (np.array([len(e) for e in entries]) > 0))[ids].sum(),
            "accepted vxlan tunnel": ((tun["kind"] == abi.TUN_VXLAN) & accepted & (self.tunnels[2] > 0))[ids].sum(),
            "accepted gre tunnel": ((tun["kind"] == abi.TUN_GRE) & accepted & (self.tunnels[2] > 0))[ids].sum(),
            "fix-up fixed == BOTH": (self.fixup[1]["done"] == BOTH)[ids].sum(),
            "decoded tcp option list": (self.options["n_tcp"] > 0)[ids].sum(),
            "flow key with ports": np.isin(self.flows["kind"], (abi.FLOW_IPV4_L4, abi.FLOW_IPV6_L4))[ids].sum(),
        }
        hit = sorted((int((sel & (rule == r))[ids].sum()) for r in range(len(FILTER.rules))), reverse=True)
        out["select: the third most hit rule"] = hit[2]
        for mode in (False, True):
            m = self.match(mode)
            out[f"match row with a mask and a first_off (frame={mode})"] = ((m["mask"] != 0) & (m["first_off"] != 0))[ids].sum()
        for inc in (False, True):
            out[f"rewrite fixed == BOTH (incremental={inc})"] = (self.rewrite(inc)[1]["fixed"] == BOTH)[ids].sum()
        return {k: int(v) for k, v in out.items()}

    def keys_per_hash(self, ids):
        """flow hash -> the distinct flow keys (kind, proto, key bytes) among the frames `ids`."""
        from nex_amd.flow import flow_key
        seen = {}
        for i in sorted(set(int(x) for x in ids)):
            kind, proto, _, key = flow_key(self.frames[i], self.recs[i], len(self.frames[i]), FLOW_OPTION)
            if kind != abi.FLOW_NONE:
                seen.setdefault(int(self.flows["hash"][i]), set()).add((kind, proto, bytes(key)))
        return seen


@functools.lru_cache(maxsize=None)
def expect():
    return Expect(far())
