"""Flow keys, the Toeplitz RSS hash, the flow-affine partition, the per-flow
counters and the flow table across batches (nexg_flow_batch /
nexg_flow_partition / nexg_flow_sort / nexg_flow_groups /
nexg_flow_table_merge, include/nexg.h; an extension: the reference has no
flow notion).

FlowOption is the host form of struct nexg_flow_option. toeplitz, flow_host,
partition_host, sort_host, groups_host and merge_host restate the header's
specification in plain Python: the GPU kernels are tested against them, and
they are themselves pinned by the published RSS verification vectors
(tests/golden/flow_vectors.json), an independent group-by
(tests/test_flow_groups_host.py) and an independent per-hash dictionary fed
frame by frame (tests/test_flow_table_host.py)."""
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

from . import abi

#: the Microsoft RSS verification key (NEXG_FLOW_DEFAULT_KEY)
DEFAULT_KEY = bytes.fromhex("6d5a56da255b0ec24167253d43a38fb0d0ca2bcbae7b30b477cb2da38030f20c6a42b73bbeac01fa")


@dataclass
class FlowOption:
    """struct nexg_flow_option. symmetric: both directions of a conversation
    get one key; ports=False: addresses only; key: 40 bytes instead of
    DEFAULT_KEY. `flags` / `reserved` set the raw fields (tests of what the
    library rejects)."""
    symmetric: bool = False
    ports: bool = True
    key: Optional[bytes] = None
    flags: Optional[int] = None  # raw nexg_flow_option.flags; None = from the fields above
    reserved: int = 0

    def raw_flags(self) -> int:
        if self.flags is not None:
            return self.flags
        return ((abi.FLOW_SYMMETRIC if self.symmetric else 0) | (0 if self.ports else abi.FLOW_NO_PORTS) |
                (abi.FLOW_KEY if self.key is not None else 0))

    def the_key(self) -> bytes:
        return DEFAULT_KEY if not self.raw_flags() & abi.FLOW_KEY or self.key is None else bytes(self.key)

    def validate(self) -> "FlowOption":
        if self.raw_flags() & ~abi.FLOW_ALL:
            raise ValueError("flow option: unknown flag bits")
        if self.reserved:
            raise ValueError("flow option: reserved must be 0")
        if self.key is not None and len(self.key) != 40:
            raise ValueError("flow option: the key is 40 bytes")
        return self

    def to_c(self, validate=True) -> abi.FlowOptionC:
        if validate:
            self.validate()
        c = abi.FlowOptionC()
        c.flags = self.raw_flags() & 0xFFFFFFFF
        c.reserved = self.reserved & 0xFFFFFFFF
        if self.key is not None:
            c.key[:] = list(bytes(self.key)[:40].ljust(40, b"\0"))
        return c


def toeplitz(data: bytes, key: bytes = DEFAULT_KEY) -> int:
    """The Toeplitz RSS hash: for every set bit s of `data` (bit 0 = the most
    significant bit of byte 0) XOR in the 32 key bits K[s, s + 32)."""
    nbits = 8 * len(key)
    if 8 * len(data) + 31 > nbits:
        raise ValueError("key too short for the input")
    k = int.from_bytes(key, "big")
    h = 0
    for s in range(8 * len(data)):
        if data[s >> 3] & (0x80 >> (s & 7)):
            h ^= (k >> (nbits - 32 - s)) & 0xFFFFFFFF
    return h


def flow_key(frame: Optional[bytes], rec, length: int, option: FlowOption = FlowOption()):
    """(kind, proto, swapped, key bytes) of one frame; kind FLOW_NONE with empty
    key bytes for a frame without a flow. `rec` is the frame's nexg_record (a
    numpy record or a dict), `frame` its bytes (None when the extent is not
    inside the batch's data), `length` len(i) as the frame table gives it."""
    fl = option.raw_flags()
    flags = int(rec["flags"])
    none = (abi.FLOW_NONE, 0, 0, b"")
    if (flags >> abi.STATUS_SHIFT) & 7:
        return none
    if flags & abi.L_IPV4:
        v6 = False
        src, dst = int(rec["ip_src"]).to_bytes(4, "big"), int(rec["ip_dst"]).to_bytes(4, "big")
    elif flags & abi.L_IPV6:
        l3 = int(rec["l3_off"])
        if frame is None or length > 65535 or l3 + 40 > length:
            return none
        v6 = True
        src, dst = bytes(frame[l3 + 8: l3 + 24]), bytes(frame[l3 + 24: l3 + 40])
    else:
        return none
    l4 = bool(flags & (abi.L_TCP | abi.L_UDP)) and not fl & abi.FLOW_NO_PORTS
    if not v6 and int(rec["ip_word"]) & 0x3FFF:  # MF or a fragment offset: NICs hash fragments on the addresses
        l4 = False
    sp = int(rec["src_port"]).to_bytes(2, "big") if l4 else b""
    dp = int(rec["dst_port"]).to_bytes(2, "big") if l4 else b""
    swapped = 0
    if fl & abi.FLOW_SYMMETRIC and src + sp > dst + dp:
        src, dst, sp, dp, swapped = dst, src, dp, sp, 1
    kind = (abi.FLOW_IPV6 if v6 else abi.FLOW_IPV4) + (1 if l4 else 0)
    return kind, int(rec["ip_proto"]), swapped, src + dst + sp + dp


def flow_host(frame: Optional[bytes], record, length: int, option: FlowOption = FlowOption()) -> Tuple[int, int, int, int]:
    """nexg_flow_batch's row for one frame: (hash, kind, proto, swapped)."""
    kind, proto, swapped, key = flow_key(frame, record, length, option)
    if kind == abi.FLOW_NONE:
        return 0, abi.FLOW_NONE, 0, 0
    return toeplitz(key, option.the_key()), kind, proto, swapped


def flows_host(frames: Sequence[Optional[bytes]], records, lengths: Sequence[int], option: FlowOption = FlowOption()):
    """flow_host over a batch as an abi.FLOW_DTYPE array."""
    out = np.zeros(len(frames), abi.FLOW_DTYPE)
    for i, fr in enumerate(frames):
        out[i] = flow_host(fr, records[i], int(lengths[i]), option) + (0,)
    return out


def partition_host(hashes, buckets: int):
    """nexg_flow_partition on the host: (index u32 [count], bucket_first i64
    [buckets + 1]) with bucket(i) = hashes[i] % buckets, the index ordered by
    bucket, then by frame number."""
    if not 1 <= buckets <= 256:
        raise ValueError("buckets must be 1..256")
    b = np.asarray(hashes, np.uint32).astype(np.int64) % buckets
    index = np.argsort(b, kind="stable").astype(np.uint32)
    first = np.zeros(buckets + 1, np.int64)
    first[1:] = np.cumsum(np.bincount(b, minlength=buckets))
    return index, first


def sort_host(hashes):
    """nexg_flow_sort on the host: the frame numbers (u32 [count]) ordered by
    (hash ascending, frame number ascending)."""
    return np.argsort(np.asarray(hashes, np.uint32), kind="stable").astype(np.uint32)


def groups_host(frames: Sequence[Optional[bytes]], records, lengths: Sequence[int], flows,
                option: FlowOption = FlowOption(), order=None):
    """nexg_flow_groups on the host: (groups, group_of, n_groups) with groups
    an abi.FLOW_GROUP_DTYPE array of one row per maximal run of equal
    flows[order[k]].hash in `order` (None: sort_host of the hashes), group_of
    (u32 [count]) the group number of every frame that `order` names (others
    keep 0xFFFFFFFF). frames / records / lengths as flows_host takes them: a
    frame is None when its extent is not inside the batch's data, and then (or
    with a length over 65535) it adds nothing to `bytes`. An order entry past
    the batch is a frame with an all-zero flow row, no key and length 0."""
    count = len(frames)
    flows = np.asarray(flows).view(abi.FLOW_DTYPE).reshape(-1)
    order = sort_host(flows["hash"]) if order is None else np.asarray(order, np.uint32)
    none = (abi.FLOW_NONE, 0, b"")
    zero = np.zeros(1, abi.FLOW_DTYPE)[0]
    keys = {}

    def member(i):
        """(flow row, key, length) of order entry i"""
        if i >= count:
            return zero, none, 0
        if i not in keys:
            kind, proto, _, key = flow_key(frames[i], records[i], int(lengths[i]), option)
            keys[i] = none if kind == abi.FLOW_NONE else (kind, proto, key)
        ln = int(lengths[i])
        return flows[i], keys[i], ln if frames[i] is not None and ln <= 65535 else 0

    rows = []
    group_of = np.full(count, 0xFFFFFFFF, np.uint32)
    prev = None
    for k, i in enumerate(int(x) for x in order[:count]):
        row, key, ln = member(i)
        if prev is None or int(row["hash"]) != prev[0]:
            rows.append(dict(hash=int(row["hash"]), kind=int(row["kind"]), proto=int(row["proto"]), first=k, packets=0,
                             bytes=0, mixed=0, first_index=i))
        elif key != prev[1]:
            rows[-1]["mixed"] += 1
        rows[-1]["packets"] += 1
        rows[-1]["bytes"] += ln
        if i < count:
            group_of[i] = len(rows) - 1
        prev = (int(row["hash"]), key)
    out = np.zeros(len(rows), abi.FLOW_GROUP_DTYPE)
    for g, r in enumerate(rows):
        out[g] = (r["hash"], r["kind"], r["proto"], abi.FLOW_GROUP_MIXED if r["mixed"] else 0, 0, r["first"], r["packets"],
                  r["bytes"], r["mixed"], r["first_index"])
    return out, group_of, len(rows)


def merge_host(table, groups, frames: Sequence[Optional[bytes]], records, lengths: Sequence[int],
               option: FlowOption = FlowOption(), epoch: int = 0, min_epoch: int = 0):
    """nexg_flow_table_merge on the host: (table_out, slot). `table` is an
    abi.FLOW_ENTRY_DTYPE array strictly ascending by hash, `groups` the
    abi.FLOW_GROUP_DTYPE rows of one batch (groups_host's, strictly ascending
    by hash), frames / records / lengths that batch as flows_host takes it.
    table_out is their union by hash, ascending, slot (u32 [n_groups]) the
    position of every group's entry in it.

    A hash in both keeps the table's entry, adds the group's packets and
    bytes, sets last_epoch = epoch, and sets MIXED when it was set, when the
    group's flags8 bit 0 is set, or when the group's key (kind, proto, the 36
    zero-padded key bytes of frame first_index; a first_index past the batch
    is a frame without a flow) differs from the entry's. A hash only in the
    groups makes an entry of the group with that key. A hash only in the table
    is kept when last_epoch >= min_epoch and dropped otherwise."""
    table = np.asarray(table).view(abi.FLOW_ENTRY_DTYPE).reshape(-1)
    groups = np.asarray(groups).view(abi.FLOW_GROUP_DTYPE).reshape(-1)
    count = len(frames)

    def group_key(g):
        i = int(g["first_index"])
        kind, proto, key = abi.FLOW_NONE, 0, b""
        if i < count:
            kind, proto, _, key = flow_key(frames[i], records[i], int(lengths[i]), option)
        return kind, proto, np.frombuffer(bytes(key).ljust(36, b"\0"), np.uint8)

    out = []
    slot = np.zeros(len(groups), np.uint32)
    i = j = n_out = 0
    while i < len(table) or j < len(groups):
        # ties: the table's entry comes first and takes its group with it
        if j == len(groups) or (i < len(table) and int(table[i]["hash"]) <= int(groups[j]["hash"])):
            e = table[i].copy()
            i += 1
            matched = j < len(groups) and int(groups[j]["hash"]) == int(e["hash"])
            if matched:
                g = groups[j]
                kind, proto, key = group_key(g)
                differs = kind != int(e["kind"]) or proto != int(e["proto"]) or not (key == e["key"]).all()
                mixed = bool(int(e["flags8"]) & abi.FLOW_ENTRY_MIXED) or \
                    bool(int(g["flags8"]) & abi.FLOW_GROUP_MIXED) or differs
                e["flags8"] = (int(e["flags8"]) & ~abi.FLOW_ENTRY_MIXED) | (abi.FLOW_ENTRY_MIXED if mixed else 0)
                e["packets"] += np.uint64(g["packets"])
                e["bytes"] += np.uint64(g["bytes"])
                e["last_epoch"] = epoch
                slot[j] = n_out
                j += 1
            keep = matched or int(e["last_epoch"]) >= min_epoch
            if keep:
                out.append(e)
            n_out += 1 if keep else 0
        else:
            g = groups[j]
            kind, proto, key = group_key(g)
            e = np.zeros(1, abi.FLOW_ENTRY_DTYPE)[0]
            e["hash"], e["kind"], e["proto"] = g["hash"], kind, proto
            e["flags8"] = int(g["flags8"]) & abi.FLOW_GROUP_MIXED
            e["key"] = key
            e["last_epoch"], e["packets"], e["bytes"] = epoch, g["packets"], g["bytes"]
            slot[j] = n_out
            out.append(e)
            n_out += 1
            j += 1
    res = np.zeros(len(out), abi.FLOW_ENTRY_DTYPE)
    for k, e in enumerate(out):
        res[k] = e
    return res, slot
