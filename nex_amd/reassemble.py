"""Host side of IPv4 reassembly (include/nexg.h nexg_reasm_plan /
nexg_reasm_frames / nexg_reasm_held): the way back from
nex_amd.fragment.fragment_host.

reassemble_host restates the contract of include/nexg.h in plain Python, a
dict group-by on the exact key, and is what the device output is tested
against (tests/test_reasm_host.py pins it by an independent reference and the
oracle's parse). The device groups by (hash, identification) and gives up on a
run whose exact keys differ; reassemble_host(exact=True) resolves those runs
and says which frames they are, reassemble_host(exact=False) gives the rows
the device gives.

    frames, src, rows, collided = reassemble_host(pieces)

Reassembler drives the device pass: run() is stateless, push() carries the
fragments of incomplete datagrams from batch to batch.
"""
from typing import List, Optional, Sequence

import numpy as np

from . import abi
from .flow import toeplitz
from .fragment import _be16, header_checksum, plan_host  # noqa: F401  (plan_host: the offsets of the outputs)


def classify_frame(frame: Optional[bytes]):
    """Rules 1-4 of include/nexg.h for one frame: (status, kind, hl, fo, mf, d,
    key). kind is REASM_NONE, REASM_PASS, or REASM_HELD for a fragment (the
    datagram decides the rest); key is (source, destination, protocol,
    identification) of a fragment, else None. `frame` None, or longer than
    65535 bytes: an extent the table does not hold."""
    if frame is None or len(frame) > 65535:
        return abi.ERR_BAD_EXTENT, abi.REASM_NONE, 0, 0, 0, 0, None
    f = bytes(frame)
    n = len(f)
    passed = (abi.FRAME_OK, abi.REASM_PASS, 0, 0, 0, 0, None)
    if n < 34 or _be16(f, 12) != 0x0800 or f[14] >> 4 != 4 or f[14] & 15 < 5:
        return passed
    hl = 4 * (f[14] & 15)
    if 14 + hl > n:
        return passed
    total = _be16(f, 16)
    if total < hl or 14 + total > n:
        return passed
    word = _be16(f, 20)
    if word & 0x3FFF == 0:
        return passed
    key = (f[26:30], f[30:34], f[23], _be16(f, 18))
    return abi.FRAME_OK, abi.REASM_HELD, hl, word & 0x1FFF, (word >> 13) & 1, total - hl, key


def key_hash(key) -> int:
    """The hash the device sorts by: Toeplitz with the default key over source,
    destination, 0, protocol, 0, 0. The identification is not hashed."""
    return toeplitz(bytes(key[0]) + bytes(key[1]) + bytes([0, key[2], 0, 0]))


def datagram_complete(members) -> bool:
    """The completeness rules of include/nexg.h. `members`: (hl, fo, mf, d) of
    each member, ordered by (fo, frame number)."""
    if members[0][1] != 0:
        return False
    for (_, fo0, mf0, d0), (_, fo1, _, _) in zip(members, members[1:]):
        if 8 * fo1 != 8 * fo0 + d0 or d0 < 8:
            return False
        if not mf0:
            return False
    hl_last, fo_last, mf_last, d_last = members[-1]
    if mf_last or d_last < 1:
        return False
    return members[0][0] + 8 * fo_last + d_last <= 65535


def rebuild(frames: Sequence[bytes], order: Sequence[int], members) -> bytes:
    """The output frame of a complete datagram: the head's Ethernet and IPv4
    header with total length, flags / offset and checksum fixed, then every
    member's data at 8 fo."""
    head = bytes(frames[order[0]])
    hl0 = members[0][0]
    size = 8 * members[-1][1] + members[-1][3]
    h = bytearray(head[14:14 + hl0])
    h[2:4] = (hl0 + size).to_bytes(2, "big")
    h[6:8] = (_be16(h, 6) & 0xC000).to_bytes(2, "big")
    h[10:12] = header_checksum(bytes(h)).to_bytes(2, "big")
    data = bytearray(size)
    for i, (hl, fo, _, d) in zip(order, members):
        data[8 * fo:8 * fo + d] = bytes(frames[i])[14 + hl:14 + hl + d]
    return head[:14] + bytes(h) + bytes(data)


def reassemble_host(frames: Sequence[Optional[bytes]], align: int = 1, exact: bool = True):
    """nexg_reasm_plan + nexg_reasm_frames in plain Python: (out, src_index,
    rows, collided). out: every output frame in order; src_index[f]: the PASS
    or HEAD input frame of output frame f; rows: an abi.REASM_DTYPE array, one
    per input frame; collided: per input frame, whether it is in a run of
    equal (hash, identification) whose exact keys differ. With exact=False
    those frames are HELD with REASM_COLLISION, as on the device; with
    exact=True they are grouped by their exact keys, and the rows differ from
    the device's at the collided frames only. `frames`: bytes, or None for an
    extent outside the data. `align` is validated as the C entries do (the
    bytes do not depend on it: see pack_host)."""
    if align not in abi.GATHER_ALIGNS:
        raise ValueError("reassemble: align must be 1, 4, 8 or 16")
    n = len(frames)
    rows = np.zeros(n, abi.REASM_DTYPE)
    rows["out"] = abi.REASM_NO_INDEX
    rows["head"] = abi.REASM_NO_INDEX
    collided = np.zeros(n, bool)
    cls = [classify_frame(f) for f in frames]
    groups = {}
    runs = {}
    for i, (status, kind, hl, fo, mf, d, key) in enumerate(cls):
        rows[i]["status"], rows[i]["kind"], rows[i]["hdr_len"] = status, kind, hl
        if key is not None:
            groups.setdefault(key, []).append(i)
            runs.setdefault((key_hash(key), key[3]), set()).add(key)
    built = {}  # head -> output frame
    for key, idx in groups.items():
        if len(runs[(key_hash(key), key[3])]) > 1:
            collided[idx] = True
            if not exact:
                rows["flags"][idx] = abi.REASM_COLLISION
                continue
        order = sorted(idx, key=lambda i: (cls[i][3], i))
        members = [cls[i][2:6] for i in order]
        if not datagram_complete(members):
            continue
        head = order[0]
        rows["kind"][order] = abi.REASM_PART
        rows["head"][order] = head
        rows[head]["kind"] = abi.REASM_HEAD
        rows[head]["members"] = len(order)
        rows[head]["data_len"] = 8 * members[-1][1] + members[-1][3]
        built[head] = rebuild(frames, order, members)
    out: List[bytes] = []
    src: List[int] = []
    for i in range(n):
        if rows[i]["kind"] == abi.REASM_PASS:
            built[i] = bytes(frames[i])
        if i in built:
            rows[i]["out"] = len(out)
            out.append(built[i])
            src.append(i)
    part = rows["kind"] == abi.REASM_PART
    rows["out"][part] = rows["out"][rows["head"][part]]
    return out, np.array(src, np.uint32), rows, collided


def pack_host(out: Sequence[bytes], align: int = 1):
    """The device's out_data for these output frames: (bytes, offsets), each
    frame's start rounded up to `align` and the pads zero."""
    offs = plan_host([len(f) for f in out], align)
    data = bytearray(int(offs[-1]))
    for f, o in zip(out, offs):
        data[int(o):int(o) + len(f)] = f
    return bytes(data), offs


class Reassembler:
    """IPv4 reassembly on an Engine (nexg_reasm_plan + nexg_reasm_frames +
    nexg_reasm_held). run() is stateless. push() keeps the fragments of
    incomplete datagrams on the device between batches, each with the epoch
    it arrived in, and puts them in front of the next batch: a datagram whose
    pieces arrive in different batches comes out of the push that brings the
    last one. Fragments older than `min_epoch` are forgotten; when the held
    bytes exceed `max_held_bytes` the oldest epochs go first, counted in
    `dropped`. Every held frame is submitted again with every push, also
    those that can never complete (a run flagged REASM_COLLISION, a datagram
    held by a retransmitted duplicate): they are sorted and gathered again
    each time until one of the two limits evicts them, so a caller of push
    always sets a `min_epoch` that moves on or a `max_held_bytes`."""

    def __init__(self, engine, max_held_bytes: Optional[int] = None):
        self.engine = engine
        self.max_held_bytes = max_held_bytes
        self.dropped = 0
        self._held = None    # a packed FrameBatch, or None
        self._epochs = None  # an int32 device tensor (bit patterns of u32), one per held frame

    @property
    def held_count(self) -> int:
        return 0 if self._held is None else self._held.count

    @property
    def held_bytes(self) -> int:
        return 0 if self._held is None else int(self._held.data.numel())

    def run(self, batch, align: int = 1, stream=None):
        """Reassemble `batch` (any frame table). Returns (out_batch, src_index,
        rows, held_table): out_batch owns its data, packed (offsets only)
        with align 1, which Engine.parse, Engine.decap and Engine.fragment
        take as it stands, offsets + lengths with a larger align; src_index
        is an int32 device tensor (bit patterns of u32) with the PASS or HEAD
        input frame of each output frame, which Engine.gather_rows takes;
        rows the nexg_reasm[count] report (uint8 device tensor,
        abi.REASM_DTYPE); held_table = (index, FrameBatch) of the HELD frames
        over batch.data, in order, as Engine.select returns a selection. The
        host side runs on `stream`. Reads the totals and the held count back:
        two synchronisations of the stream."""
        with self.engine._on(stream):
            if align not in abi.GATHER_ALIGNS:
                raise ValueError("reassemble: align must be 1, 4, 8 or 16")
            return self._run(batch, align, stream)

    def _run(self, batch, align, stream):
        from .engine import FrameBatch, _frames, _ordered, _ptr, _torch
        torch = _torch()
        eng = self.engine
        dev = eng.torch_device
        n = batch.count
        first = torch.empty(n + 1, dtype=torch.int32, device=dev)
        nbytes = torch.empty(n + 1, dtype=torch.int64, device=dev)
        rows = torch.empty(max(n, 1) * 16, dtype=torch.uint8, device=dev)
        ws_bytes = abi.reasm_plan_workspace(n)
        ws = torch.empty((ws_bytes + 15) // 16 * 2, dtype=torch.int64, device=dev)
        fr = _frames(batch)
        s = eng._stream(stream)
        eng._check(eng.lib.nexg_reasm_plan(eng.ctx, fr, align, _ptr(first), _ptr(nbytes), _ptr(rows), _ptr(ws), ws_bytes, s))
        totals = torch.stack((first[n].to(torch.int64) & 0xFFFFFFFF, nbytes[n])).cpu()  # waits for the kernels
        k, total = int(totals[0]), int(totals[1])
        offs = torch.empty(k + 1, dtype=torch.int64, device=dev)
        ln = torch.empty(max(k, 1), dtype=torch.int32, device=dev)
        src = torch.empty(max(k, 1), dtype=torch.int32, device=dev)
        data = torch.empty(max(total, 16), dtype=torch.uint8, device=dev)
        eng._check(eng.lib.nexg_reasm_frames(eng.ctx, fr, align, _ptr(rows), _ptr(first), _ptr(nbytes), k, _ptr(offs),
                                             _ptr(ln), _ptr(src), _ptr(data), total, s))
        out = FrameBatch(data=data[:total], count=k, offsets=offs, lengths=None if align == 1 else ln[:k],
                         hints=0 if align == 1 else abi.FRAMES_MONOTONE)
        idx, off, hl = eng._table(n)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        hw_bytes = abi.reasm_held_workspace(n)
        hw = eng._workspace(hw_bytes)
        eng._check(eng.lib.nexg_reasm_held(eng.ctx, fr, _ptr(rows), n, _ptr(idx), _ptr(off), _ptr(hl), _ptr(cnt), _ptr(hw),
                                           hw_bytes, s))
        h = int(cnt.item())  # waits for the kernels
        held = FrameBatch(data=batch.data, count=h, offsets=off[:h], lengths=hl[:h],
                          hints=abi.FRAMES_MONOTONE if _ordered(batch) else 0)
        return out, src[:k], rows[: n * 16], (idx[:h], held)

    def push(self, batch, epoch: int, min_epoch: int = 0, stream=None):
        """run() over the fragments held from earlier pushes followed by
        `batch`, whose frames arrive in `epoch`. Returns run()'s outputs for
        that combined table (align 1): input frame numbers count the held
        frames first (held_count of them, as before this call), then the
        batch's. Afterwards the object holds the new HELD frames whose epoch
        is at least `min_epoch`, within max_held_bytes."""
        if not 0 <= int(epoch) <= 0xFFFFFFFF or not 0 <= int(min_epoch) <= 0xFFFFFFFF:
            raise ValueError("reassemble: epochs are 32-bit")
        with self.engine._on(stream):
            return self._push(batch, int(epoch), int(min_epoch), stream)

    def _push(self, batch, epoch, min_epoch, stream):
        from .engine import FrameBatch, _torch
        torch = _torch()
        eng = self.engine
        dev = eng.torch_device
        dense = eng.gather(batch, stream=stream)  # packed: offsets of count + 1 entries
        new_epochs = torch.full((dense.count,), epoch - (1 << 32) if epoch >= 1 << 31 else epoch, dtype=torch.int32, device=dev)
        if self._held is not None and self._held.count:
            held = self._held
            base = int(held.data.numel())
            whole = FrameBatch(data=torch.cat((held.data, dense.data)), count=held.count + dense.count,
                               offsets=torch.cat((held.offsets[: held.count], dense.offsets + base)))
            epochs = torch.cat((self._epochs, new_epochs))
        else:
            whole, epochs = dense, new_epochs
        out, src, rows, (hidx, htable) = self._run(whole, 1, stream)
        # which of the held frames stay: few frames, so the decision is made on the host
        ep = (eng.gather_rows(epochs, 4, hidx, stream=stream).view(torch.int32).cpu().numpy().astype(np.int64)
              & 0xFFFFFFFF)[: htable.count]
        ln = htable.lengths.cpu().numpy().astype(np.int64)[: htable.count]
        keep = ep >= min_epoch
        if self.max_held_bytes is not None:
            while keep.any() and int(ln[keep].sum()) > self.max_held_bytes:
                oldest = ep[keep].min()
                gone = keep & (ep == oldest)
                self.dropped += int(gone.sum())
                keep &= ~gone
        if keep.any():
            at = torch.from_numpy(np.flatnonzero(keep)).to(dev)
            sub = FrameBatch(data=htable.data, count=int(keep.sum()), offsets=htable.offsets[at], lengths=htable.lengths[at],
                             hints=htable.hints)
            self._held = eng.gather(sub, stream=stream)
            self._epochs = torch.from_numpy(ep[keep].astype(np.uint32).view(np.int32)).to(dev)
        else:
            self._held, self._epochs = None, None
        return out, src, rows, (hidx, htable)
