"""What the flow-table tests share (nexg_flow_table_merge, include/nexg.h): an
independent reference for a table kept over a sequence of batches, the batch
sequences the CPU and GPU tests run, and the chained host contract.

RefTable is a dict from hash to (packets, bytes, the set of keys seen, the
first key, last_epoch), fed frame by frame. Its keys are
tests.flow_group_frames.ref_key's (the header's text on
tests/second_pass_ref.py's address code), not nex_amd.flow.flow_key's, and it
knows nothing of groups, sorting or merging: only its rows() are put in hash
order, to be compared."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

from nex_amd import abi
from nex_amd.flow import FlowOption, groups_host
from tests import flow_frames as ff
from tests import flow_group_frames as fg
from tests import second_pass_ref as ref
from tests import select_frames as sf

OPTIONS = [(s, p) for s in (False, True) for p in (True, False)]
ENTRY_FIELDS = abi.FLOW_ENTRY_DTYPE.names


def option_of(symmetric, ports):
    return FlowOption(symmetric=symmetric, ports=ports)


class RefTable:
    def __init__(self, symmetric=False, ports=True):
        self.symmetric, self.ports = symmetric, ports
        self.flows = {}
        self.fed = 0

    def feed(self, frames, recs, lengths, hashes, epoch, min_epoch=0):
        """One batch, frame by frame; then the flows the batch did not touch
        and whose last_epoch is below min_epoch are forgotten."""
        touched = set()
        for i, f in enumerate(frames):
            h = int(hashes[i])
            key = fg.ref_key(f, recs[i], int(lengths[i]), self.symmetric, self.ports)
            e = self.flows.get(h)
            if e is None:
                e = self.flows[h] = dict(packets=0, bytes=0, keys=set(), first=key)
            e["packets"] += 1
            if f is not None and int(lengths[i]) <= 65535:
                e["bytes"] += int(lengths[i])
            e["keys"].add(key)
            e["last_epoch"] = epoch
            touched.add(h)
            self.fed += 1
        for h in [h for h, e in self.flows.items() if h not in touched and e["last_epoch"] < min_epoch]:
            del self.flows[h]

    def rows(self):
        out = np.zeros(len(self.flows), abi.FLOW_ENTRY_DTYPE)
        for k, h in enumerate(sorted(self.flows)):
            e = self.flows[h]
            kind, proto, key = e["first"] or (abi.FLOW_NONE, 0, b"")
            out[k] = (h, kind, proto, abi.FLOW_ENTRY_MIXED if len(e["keys"]) > 1 else 0, 0,
                      np.frombuffer(key.ljust(36, b"\0"), np.uint8), e["last_epoch"], e["packets"], e["bytes"])
        return out

    def row_of(self, hashes):
        """The row of rows() that each of the hashes has."""
        where = {h: k for k, h in enumerate(sorted(self.flows))}
        return np.array([where[int(h)] for h in hashes], np.uint32)


def entries_equal(got, want, name):
    assert len(got) == len(want), (name, len(got), len(want))
    for n in ENTRY_FIELDS if len(got) else ():
        bad = np.nonzero((got[n] != want[n]).reshape(len(got), -1).any(axis=1))[0]
        assert len(bad) == 0, (name, n, int(bad[0]), got[bad[0]], want[bad[0]])


# ---- batch sequences ---------------------------------------------------------------------------

@dataclass
class Batch:
    frames: list
    recs: np.ndarray
    lengths: np.ndarray
    epoch: int
    min_epoch: int = 0
    hashes: Optional[np.ndarray] = None  # made-up flow hashes (None: every frame's own)

    def flows(self, symmetric, ports):
        """The flow rows the batch is grouped by (second_pass_ref's, with the made-up hashes put in)."""
        rows = ref.flow_rows(self.frames, self.recs, self.lengths, symmetric, ports)
        if self.hashes is not None:
            rows["hash"] = self.hashes
        return rows


def make_batch(oracle, frames, epoch, min_epoch=0, hashes=None, lengths=None, lose=()):
    """`lose`: the frames whose bytes are taken away after the parse (an
    extent outside the data); `lengths`: what the table says, if not the truth."""
    frames = list(frames)
    recs = oracle.parse_frames(frames, ff.PARSE_FLAGS)
    lengths = np.array([len(f) for f in frames] if lengths is None else lengths)
    for i in lose:
        frames[i] = None
    return Batch(frames, recs, lengths, epoch, min_epoch, None if hashes is None else np.asarray(hashes, np.uint32))


def corpus_frames():
    return [x.frame for x in ff.corpus()] + fg.collision_frames()


def sequences(oracle):
    """name -> [Batch, ...]: the cases the merge's rules are about."""
    A, B = fg.collision_frames("AB")
    own = [x.frame for x in ff.own_corpus()]
    arp = next(x.frame for x in ff.own_corpus() if x.what == "arp")
    udp = ff._tuple("udp", ff.A4, ff.B4, 1111, 2222, "udp").frame
    tcp = ff._tuple("tcp", ff.A4, ff.B4, 1111, 2222, "tcp").frame
    udp00 = ff._tuple("udp", ff.A4, ff.B4, 0, 0, "udp ports 0").frame
    later = sf.eth(ff.ip4_frag(ff.A4, ff.B4, 17, bytes(24), frag_off=3))  # a UDP fragment: no ports in its key
    other = ff._tuple("udp", "10.9.9.9", "10.8.8.8", 5, 6, "another flow").frame
    third = ff._tuple("tcp", "10.7.7.7", "10.6.6.6", 7, 8, "a third flow").frame
    mk = lambda *a, **k: make_batch(oracle, *a, **k)
    corpus = corpus_frames()
    n = len(corpus)
    cut = [0, n // 4, n // 4 + n // 3, n - 7, n]
    seq = {
        # 4 batches cut from the corpus, the last one the first one's frames again
        "corpus, nothing expires": [mk(corpus[cut[k]: cut[k + 1]], k) for k in range(4)] + [mk(corpus[: cut[1]], 4)],
        "corpus, a timeout of one epoch": [mk(corpus[cut[k]: cut[k + 1]], k + 3, k + 2) for k in range(4)] +
                                          [mk(corpus[: cut[1]], 9, 7)],
        "collision: A then B": [mk([A, other], 1), mk([B], 2)],
        "collision: A then A": [mk([A, other], 1), mk([A, A], 2)],
        "collision: A, B, then A again": [mk([A], 1), mk([B, other], 2), mk([A], 3)],
        "collision inside a batch, then carried": [mk([A, B, A], 1), mk([other], 2), mk([A], 3)],
        "no flow, then a real flow under hash 0": [mk([arp, other], 1), mk([udp, third], 2, hashes=[0, 0x51CCC17D])],
        "a real flow under hash 0, then no flow": [mk([udp], 1, hashes=[0]), mk([arp], 2)],
        "same key bytes, another protocol": [mk([udp], 1), mk([tcp], 2)],
        "same padded key bytes, another kind": [mk([later, other], 1), mk([udp00], 2)],
        # the table holds epochs 5 (other), 6 (udp), 7 (third): at min_epoch 6 `other` goes although ...
        "expiry: equal is kept, one below is dropped": [mk([other], 5), mk([udp], 6), mk([third], 7),
                                                        mk([A], 8, min_epoch=6)],
        # ... and here it stays, old as it is, because the batch has it
        "expiry: an old entry that is matched stays": [mk([other], 5), mk([udp], 6), mk([third], 7),
                                                      mk([other, A], 8, min_epoch=7)],
        "expiry: everything old goes, the batch's own flows stay": [mk(own[:20], 1), mk(own[20:30], 2),
                                                                    mk(own[5:8], 9, min_epoch=9)],
        "an empty batch expires": [mk(own[:10], 1), mk(own[10:20], 2), mk([], 3, min_epoch=2)],
        "an empty batch into an empty table": [mk([], 1)],
        # bad extents: no bytes for the frame (its IPv6 key is gone too), a length over 65535
        "bad extents": [mk(own, 1, lose=range(2, len(own), 5),
                           lengths=[len(f) + (65536 if i % 7 == 3 else 0) for i, f in enumerate(own)]), mk(own, 2)],
    }
    return seq


def run_reference(batches, symmetric, ports):
    """Per batch: (RefTable rows, the row of every frame's flow)."""
    t = RefTable(symmetric, ports)
    out = []
    for b in batches:
        hashes = b.flows(symmetric, ports)["hash"]
        t.feed(b.frames, b.recs, b.lengths, hashes, b.epoch, b.min_epoch)
        out.append((t.rows(), t.row_of(hashes)))
    return out, t.fed


def run_host(merge, batches, symmetric, ports):
    """Per batch: (table, the row of every frame's entry) of `merge`
    (nex_amd.flow.merge_host or a variant of it) chained over the batches."""
    option = option_of(symmetric, ports)
    table = np.zeros(0, abi.FLOW_ENTRY_DTYPE)
    out = []
    for b in batches:
        groups, group_of, _ = groups_host(b.frames, b.recs, b.lengths, b.flows(symmetric, ports), option)
        table, slot = merge(table, groups, b.frames, b.recs, b.lengths, option, b.epoch, b.min_epoch)
        out.append((table, slot[group_of] if len(group_of) else np.zeros(0, np.uint32)))
    return out
