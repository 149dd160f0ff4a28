"""Batched device engine over the C ABI (include/nexg.h).

torch is used only as device-memory / stream plumbing: frames, offsets and
outputs are torch CUDA(HIP) tensors whose data pointers go straight to
libnexg.so, and work is enqueued on torch's current stream, or on the
`stream` a pass is given: its kernels, allocations and read-backs alike.
"""
import contextlib
import ctypes
import functools
import inspect
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import abi
from ._lib import load
from .frame import ParseMode, ParseOption


class NexgError(RuntimeError):
    def __init__(self, status, message=""):
        super().__init__(f"nexg error {status}: {message}")
        self.status = status


def _torch():
    import torch
    return torch


_CURRENT = contextlib.nullcontext()  # stateless, so one serves every call


def _on_stream(fn):
    """Run a method that takes `stream` under Engine._on(stream): what its
    body allocates, fills, reduces and reads back through torch is then in
    `stream`'s order and from its allocator pool, like the kernels it
    enqueues there. With stream=None the method is called as it stands."""
    at = list(inspect.signature(fn).parameters).index("stream") - 1  # in *args, which leaves self out

    @functools.wraps(fn)
    def method(self, *args, **kwargs):
        stream = args[at] if len(args) > at else kwargs.get("stream")
        if stream is None:
            return fn(self, *args, **kwargs)
        with self._on(stream):
            return fn(self, *args, **kwargs)
    return method


def u32_tensor(values, device="cuda"):
    """Device tensor holding u32 values (stored as int32 bit patterns)."""
    a = np.asarray(values, dtype=np.uint64).astype(np.uint32).view(np.int32)
    return _torch().from_numpy(np.ascontiguousarray(a)).to(device)


def u16_tensor(values, device="cuda"):
    """Device tensor holding u16 values (stored as int16 bit patterns)."""
    a = np.asarray(values, dtype=np.uint64).astype(np.uint16).view(np.int16)
    return _torch().from_numpy(np.ascontiguousarray(a)).to(device)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _frames(batch):
    """The nexg_frames argument of a call (it keeps the structure alive)."""
    return ctypes.byref(batch.to_c())


def _ordered(batch):
    """Whether a table derived from `batch` frame by frame is monotone: the
    batch is fixed-stride, packed or itself carries FRAMES_MONOTONE."""
    return batch.offsets is None or batch.lengths is None or bool(batch.hints & abi.FRAMES_MONOTONE)


@dataclass
class FrameBatch:
    """A device-resident batch of raw frames (nexg_frames).

    data     uint8 tensor on the device
    offsets  int64 tensor (count or count+1 entries), or a uint8 tensor
             holding a NEXG_FRAMES_OFFSETS32 table (abi.offsets32_table;
             hints must carry abi.FRAMES_OFFSETS32), or None (fixed stride)
    lengths  int32 tensor or None
    """
    data: "object"
    count: int
    stride: int = 0
    offsets: Optional[object] = None
    lengths: Optional[object] = None
    hints: int = 0  # abi.FRAMES_* (nexg_frames.hints)
    bucket_hints: int = 0  # Engine.flow_partition's table: the hints of each bucket's view (Engine.flow_bucket)

    def to_c(self):
        return abi.Frames(
            data=self.data.data_ptr() if self.count else None,
            data_bytes=self.data.numel(),
            offsets=None if self.offsets is None else self.offsets.data_ptr(),
            lengths=None if self.lengths is None else self.lengths.data_ptr(),
            stride=self.stride, hints=self.hints, count=self.count)

    def host_offsets(self):
        """Host int64 array of the table's offsets (count + 1 entries for a
        packed batch), decoding a NEXG_FRAMES_OFFSETS32 table."""
        if self.hints & abi.FRAMES_OFFSETS32:
            return abi.offsets32_decode(self.offsets.cpu().numpy(), self.count,
                                        self.data.numel()).astype(np.int64)
        return self.offsets.cpu().numpy().astype(np.int64)

    def frame_lengths(self):
        """Host int64 array of every frame's length (the nexg_frames rules)."""
        if self.lengths is not None:
            return self.lengths[: self.count].cpu().numpy().astype(np.int64)
        if self.offsets is not None:
            return np.diff(self.host_offsets()[: self.count + 1])
        return np.full(self.count, self.stride, np.int64)

    @property
    def total_bytes(self):
        if self.lengths is not None:
            return int(self.lengths.sum().item())
        if self.offsets is not None and self.hints & abi.FRAMES_OFFSETS32:
            o = self.host_offsets()
            return int(o[self.count] - o[0])
        if self.offsets is not None:
            return int((self.offsets[self.count] - self.offsets[0]).item())
        return self.count * self.stride

    def with_offsets32(self):
        """The same frames described by a NEXG_FRAMES_OFFSETS32 table (4 B per
        frame instead of 8, plus one 8-B base per 256 frames over 4 GiB)."""
        torch = _torch()
        assert self.offsets is not None and not self.hints & abi.FRAMES_OFFSETS32
        n = self.count + (0 if self.lengths is not None else 1)
        o = self.offsets[:n].cpu().numpy().astype(np.uint64)
        if self.lengths is not None:  # count entries: the table still has count + 1 slots
            o = np.concatenate([o, o[-1:] if len(o) else np.zeros(1, np.uint64)])
        t = torch.from_numpy(abi.offsets32_table(o, self.data.numel())).to(self.data.device)
        return FrameBatch(data=self.data, count=self.count, stride=self.stride, offsets=t, lengths=self.lengths,
                          hints=self.hints | abi.FRAMES_OFFSETS32)

    @classmethod
    def from_frames(cls, frames: Sequence[bytes], device="cuda", pad_to=4):
        """Pack host frames back to back (each start aligned to `pad_to`)."""
        torch = _torch()
        offs = np.zeros(len(frames) + 1, dtype=np.int64)
        lens = np.array([len(f) for f in frames], dtype=np.int32)
        pos = 0
        for i, f in enumerate(frames):
            offs[i] = pos
            pos += (len(f) + pad_to - 1) // pad_to * pad_to
        offs[len(frames)] = pos
        buf = np.zeros(max(pos, 16), dtype=np.uint8)
        for i, f in enumerate(frames):
            buf[offs[i]:offs[i] + len(f)] = np.frombuffer(bytes(f), dtype=np.uint8)
        return cls(data=torch.from_numpy(buf).to(device), count=len(frames),
                   offsets=torch.from_numpy(offs).to(device),
                   lengths=torch.from_numpy(lens).to(device))

    @classmethod
    def from_packed(cls, frames: Sequence[bytes], device="cuda", pad_to=1, shift=0):
        """Offset table only (lengths implied by consecutive offsets): frames
        zero-padded to `pad_to`, back to back, starting `shift` bytes into an
        allocation (the packed layout nexg_parse_batch streams by spans)."""
        torch = _torch()
        padded = [bytes(f) + bytes((-len(f)) % pad_to) for f in frames]
        offs = np.zeros(len(padded) + 1, dtype=np.int64)
        offs[1:] = np.cumsum([len(f) for f in padded])
        buf = np.zeros(shift + int(offs[-1]) + 16, dtype=np.uint8)
        buf[shift:shift + int(offs[-1])] = np.frombuffer(b"".join(padded), dtype=np.uint8)
        dev = torch.from_numpy(buf).to(device)
        return cls(data=dev[shift:shift + int(offs[-1])], count=len(padded),
                   offsets=torch.from_numpy(offs).to(device))

    @classmethod
    def from_strided(cls, array: np.ndarray, device="cuda", lengths=None):
        """count x stride uint8 host array -> fixed-stride device batch."""
        torch = _torch()
        count, stride = array.shape
        data = torch.from_numpy(np.ascontiguousarray(array).reshape(-1)).to(device)
        lt = None if lengths is None else torch.from_numpy(np.asarray(lengths, np.int32)).to(device)
        return cls(data=data, count=count, stride=stride, lengths=lt)


class Engine:
    """One nexg context bound to one gfx950 device (nexg_ctx_create)."""

    def __init__(self, device: int = 0):
        self.lib = load()
        torch = _torch()
        self.device = device
        self.torch_device = torch.device("cuda", device)
        h = ctypes.c_void_p()
        rc = self.lib.nexg_ctx_create(device, ctypes.byref(h))
        if rc != abi.OK:
            raise NexgError(rc, self.lib.nexg_strerror(rc).decode())
        self.ctx = h

    def close(self):
        if self.ctx:
            self.lib.nexg_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def cu_count(self):
        return self.lib.nexg_ctx_cu_count(self.ctx)

    def _stream(self, stream):
        torch = _torch()
        s = stream if stream is not None else torch.cuda.current_stream(self.torch_device)
        return ctypes.c_void_p(s.cuda_stream)

    def _on(self, stream):
        """The context a pass's host side runs in: torch.cuda.stream(stream),
        or nothing to enter when `stream` is None or already current."""
        torch = _torch()
        if stream is None or stream == torch.cuda.current_stream(self.torch_device):
            return _CURRENT
        return torch.cuda.stream(stream)

    def _check(self, rc):
        if rc != abi.OK:
            raise NexgError(rc, self.lib.nexg_ctx_last_error(self.ctx).decode())

    def _table(self, count):
        """The (index, off, len) tensors of a derived table: max(count, 1) rows."""
        torch = _torch()
        n, dev = max(count, 1), self.torch_device
        return (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int64, device=dev),
                torch.empty(n, dtype=torch.int32, device=dev))

    def _workspace(self, nbytes):
        """A workspace of at least `nbytes`, 8-B aligned."""
        return _torch().empty((nbytes + 7) // 8, dtype=_torch().int64, device=self.torch_device)

    @_on_stream
    def _compact(self, fn, table: FrameBatch, hints, *, before, after=(), stream=None):
        """What the three selects share. Calls

            fn(ctx, *before, index, off, len, *after, count, workspace, workspace bytes, stream)

        with fn one of nexg_decap_select, nexg_select_batch and
        nexg_match_select, fresh (index, off, len) outputs for table.count
        rows and a workspace of abi.select_workspace bytes (the one formula of
        all three), then reads the selected count k back. Returns (index,
        FrameBatch): the first k rows of the outputs over table.data, with
        `hints`."""
        torch = _torch()
        count = table.count
        idx, off, ln = self._table(count)
        cnt = torch.zeros(1, dtype=torch.int64, device=self.torch_device)
        ws_bytes = abi.select_workspace(count)
        ws = self._workspace(ws_bytes)
        self._check(fn(self.ctx, *before, _ptr(idx), _ptr(off), _ptr(ln), *after, _ptr(cnt), _ptr(ws), ws_bytes,
                       self._stream(stream)))
        k = int(cnt.item())  # waits for the kernels
        return idx[:k], FrameBatch(data=table.data, count=k, offsets=off[:k], lengths=ln[:k], hints=hints)

    # --- hot path -------------------------------------------------------
    @_on_stream
    def parse(self, batch: FrameBatch, option: ParseOption = ParseOption(),
              mode: ParseMode = ParseMode.Lenient, out_kind: int = abi.OUT_DESC,
              out=None, stream=None):
        """Frame::try_from_buf_with_mode on every frame (frame.rs:309), or
        FrameSlice::try_from_buf (frame.rs:86) with out_kind=OUT_SLICE.

        Returns a uint8 device tensor holding nexg_desc[count] (8 B each),
        nexg_record[count] (64 B), nexg_slice[count] (16 B) or, with
        out_kind=OUT_FLAGS, the nexg_desc.flags word alone (4 B), or with
        OUT_VERDICT its lossless 2-B form (abi.verdict_to_flags)."""
        torch = _torch()
        nbytes = self.out_bytes(out_kind, batch.count)
        if out is None:
            out = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self.torch_device)
        elif out.numel() * out.element_size() < nbytes or out.device != self.torch_device:
            raise ValueError(f"out holds {out.numel() * out.element_size()} B on {out.device}; "
                             f"{nbytes} B on {self.torch_device} needed")
        opt = abi.ParseOptionC(option.flags(mode), option.offset)
        self._check(self.lib.nexg_parse_batch(self.ctx, _frames(batch), ctypes.byref(opt), out_kind,
                                              _ptr(out), self._stream(stream)))
        return out

    @staticmethod
    def out_bytes(out_kind, count):
        """Bytes of a nexg_parse_batch output of `out_kind` for `count` frames."""
        if out_kind == abi.OUT_SPARSE:
            return abi.sparse_bytes(count)
        if out_kind == abi.OUT_GROUPED:
            return abi.grouped_offsets(count)[3]
        return count * {abi.OUT_DESC: 8, abi.OUT_RECORD: 64, abi.OUT_SLICE: 16, abi.OUT_FLAGS: 4,
                        abi.OUT_VERDICT: 2}[out_kind]

    def parse_to_numpy(self, batch, option=ParseOption(), mode=ParseMode.Lenient,
                       out_kind=abi.OUT_RECORD):
        """Host copy of the parse output; OUT_SPARSE / OUT_GROUPED come back
        decoded on the host into nexg_desc (abi.sparse_to_desc / grouped_to_desc)."""
        out = self.parse(batch, option, mode, out_kind)
        _torch().cuda.synchronize(self.torch_device)
        if out_kind in (abi.OUT_SPARSE, abi.OUT_GROUPED):
            dec = abi.sparse_to_desc if out_kind == abi.OUT_SPARSE else abi.grouped_to_desc
            return dec(out.cpu().numpy(), batch.count, batch.frame_lengths(), option.flags(mode), option.offset)
        dt = {abi.OUT_DESC: abi.DESC_DTYPE, abi.OUT_RECORD: abi.RECORD_DTYPE,
              abi.OUT_SLICE: abi.SLICE_DTYPE, abi.OUT_FLAGS: abi.FLAGS_DTYPE,
              abi.OUT_VERDICT: abi.VERDICT_DTYPE}[out_kind]
        return out.cpu().numpy()[: batch.count * dt.itemsize].view(dt)

    @_on_stream
    def sparse_expand(self, batch: FrameBatch, sparse, option: ParseOption = ParseOption(),
                      mode: ParseMode = ParseMode.Lenient, out=None, stream=None, grouped=False):
        """nexg_desc[count] (uint8 device tensor) from a NEXG_OUT_SPARSE output
        (grouped=True: NEXG_OUT_GROUPED) of the same batch and option
        (nexg_sparse_expand / nexg_grouped_expand)."""
        torch = _torch()
        if out is None:
            out = torch.empty(max(batch.count, 1) * 8, dtype=torch.uint8, device=self.torch_device)
        opt = abi.ParseOptionC(option.flags(mode), option.offset)
        fn = self.lib.nexg_grouped_expand if grouped else self.lib.nexg_sparse_expand
        self._check(fn(self.ctx, _frames(batch), ctypes.byref(opt), _ptr(sparse), _ptr(out), self._stream(stream)))
        return out

    @_on_stream
    def recompute_checksums(self, batch: FrameBatch, which: int = abi.FIX_IP | abi.FIX_L4,
                            option: ParseOption = ParseOption(), report=True, stream=None):
        """In-place checksum fix-up of batch.data with the mutable views'
        raw-buffer semantics (nexg_recompute_checksums_batch; ipv4.rs:669-679,
        udp.rs:338-369, tcp.rs:1009-1040, icmp.rs:372-377, icmpv6.rs:450-470).
        Returns the nexg_fixup[count] report (uint8 device tensor) or None."""
        torch = _torch()
        out = torch.empty(max(batch.count, 1) * 8, dtype=torch.uint8, device=self.torch_device) if report else None
        opt = abi.ParseOptionC(option.flags(ParseMode.Lenient), option.offset)
        self._check(self.lib.nexg_recompute_checksums_batch(self.ctx, _frames(batch), ctypes.byref(opt), which,
                                                            _ptr(out), self._stream(stream)))
        return out

    @_on_stream
    def rewrite(self, batch: FrameBatch, actions, index=None, option: ParseOption = ParseOption(), report=True,
                stream=None):
        """Header fields rewritten in place in batch.data (nexg_rewrite_batch):
        the mutable setters under ChecksumMode::Automatic — MACs, IPv4 / IPv6
        addresses, ports, TTL / hop limit, TOS / traffic class — with the
        checksums they dirty recomputed, or updated by RFC 1624 with
        ActionSet(incremental=True). `actions` is a nex_amd.rewrite.ActionSet,
        `index` a uint8 device tensor with one action number per frame
        (abi.ACTION_NONE or any number past the set: leave the frame alone) or
        None (action 0 for every frame). Returns the nexg_rewritten[count]
        rows (uint8 device tensor, abi.REWRITTEN_DTYPE) or None. One kernel,
        no synchronisation.

        The recipe, a match-action table: rule j of the filter gets action j.

            rec = eng.parse(batch, out_kind=abi.OUT_RECORD)
            idx, sel, rule = eng.select(batch, rec, flt, want_rule=True)
            eng.rewrite(sel, actions, rule)
        """
        torch = _torch()
        ac = actions.to_c()  # ValueError for what nexg_rewrite_batch rejects
        out = torch.empty(max(batch.count, 1) * 8, dtype=torch.uint8, device=self.torch_device) if report else None
        opt = abi.ParseOptionC(option.flags(ParseMode.Lenient), option.offset)
        self._check(self.lib.nexg_rewrite_batch(self.ctx, _frames(batch), ctypes.byref(opt), ctypes.byref(ac),
                                                _ptr(index), _ptr(out), self._stream(stream)))
        return out[: batch.count * 8] if report else None

    @_on_stream
    def decode_options(self, batch: FrameBatch, records, stream=None):
        """Ipv4Header.options / TcpHeader.options of every frame as positions
        (nexg_decode_options; ipv4.rs:442-508, tcp.rs:767-818). `records` is
        the uint8 device tensor a NEXG_OUT_RECORD parse of `batch` returned."""
        torch = _torch()
        out = torch.empty(max(batch.count, 1) * 96, dtype=torch.uint8, device=self.torch_device)
        self._check(self.lib.nexg_decode_options(self.ctx, _frames(batch), _ptr(records), _ptr(out),
                                                 self._stream(stream)))
        return out

    @_on_stream
    def decap(self, batch: FrameBatch, records, which: int = abi.DECAP_VXLAN | abi.DECAP_GRE,
              vxlan_port: int = abi.VXLAN_PORT, stream=None):
        """Locate every VXLAN / GRE tunnel's inner frame inside `batch`
        (nexg_decap_batch; VxlanPacket::try_from_buf vxlan.rs:28-65,
        GrePacket::try_from_buf gre.rs:32-107 on Frame.payload). `records` is
        the uint8 device tensor a NEXG_OUT_RECORD parse of `batch` returned
        (any parse option). Returns (tunnels, inner): tunnels a uint8 device
        tensor holding nexg_tunnel[count] (abi.TUNNEL_DTYPE), inner a
        FrameBatch of `count` frames that shares batch.data (no bytes are
        copied) with the inner offsets + lengths; frames that are no accepted
        tunnel have length 0. inner carries FRAMES_MONOTONE exactly when the
        outer batch is fixed-stride, packed or itself monotone.

        The two-call recipe for the inner frames:

            tunnels, inner = eng.decap(batch, records)
            idx, eth = eng.decap_select(tunnels, inner, {abi.INNER_ETHERNET})
            rec_eth = eng.parse(eth, out_kind=abi.OUT_RECORD)
            idx, ip = eng.decap_select(tunnels, inner, {abi.INNER_IPV4, abi.INNER_IPV6})
            rec_ip = eng.parse(ip, ParseOption(from_ip_packet=True, offset=0), out_kind=abi.OUT_RECORD)

        idx[k] is the outer frame of the k-th selected inner frame."""
        torch = _torch()
        n = max(batch.count, 1)
        tunnels = torch.empty(n * 16, dtype=torch.uint8, device=self.torch_device)
        off = torch.empty(n, dtype=torch.int64, device=self.torch_device)
        ln = torch.empty(n, dtype=torch.int32, device=self.torch_device)
        opt = abi.DecapOption(which, vxlan_port, 0)
        self._check(self.lib.nexg_decap_batch(self.ctx, _frames(batch), _ptr(records), ctypes.byref(opt),
                                              _ptr(tunnels), _ptr(off), _ptr(ln), self._stream(stream)))
        inner = FrameBatch(data=batch.data, count=batch.count, offsets=off[: batch.count], lengths=ln[: batch.count],
                           hints=abi.FRAMES_MONOTONE if _ordered(batch) else 0)
        return tunnels[: batch.count * 16], inner

    @_on_stream
    def decap_select(self, tunnels, inner: FrameBatch, classes, stream=None):
        """Order-preserving compaction of a decap result (nexg_decap_select):
        the accepted tunnels whose inner class (abi.INNER_*) is in `classes`.
        Returns (index, batch): index an int32 device tensor (bit patterns of
        u32) with the outer frame number of each selected inner frame, batch a
        FrameBatch over the same data whose count is the selected count, ready
        for Engine.parse: {INNER_ETHERNET} with the default option,
        {INNER_IPV4, INNER_IPV6} with ParseOption(from_ip_packet=True,
        offset=0) (see Engine.decap). Allocates the workspace and reads the
        selected count back: one synchronisation of the stream."""
        mask = 0
        for c in classes:
            mask |= 1 << int(c)
        return self._compact(self.lib.nexg_decap_select, inner, inner.hints, stream=stream,
                             before=(_ptr(tunnels), _ptr(inner.offsets), _ptr(inner.lengths), inner.count, mask))

    @_on_stream
    def select(self, batch: FrameBatch, records, flt, want_rule: bool = False, stream=None):
        """Order-preserving selection of frames by rule (nexg_select_batch;
        an extension, the reference has no filter). `records` is the uint8
        device tensor a NEXG_OUT_RECORD parse of `batch` returned (for an
        inner table from Engine.decap: the inner records), `flt` a
        nex_amd.select.Filter. Returns (index, selected[, rule]): index an
        int32 device tensor (bit patterns of u32) with the frame number of
        each selected frame, selected a FrameBatch (offsets + lengths) over
        the same data whose count is the selected count, rule (want_rule) a
        uint8 device tensor with the lowest matching rule per selected frame.
        Allocates the workspace and reads the selected count back: one
        synchronisation of the stream.

        The recipe: parse, select, compact the records, run the follow-up
        passes on the selected table only, copy out just what matched:

            rec = eng.parse(batch, out_kind=abi.OUT_RECORD)
            idx, sel = eng.select(batch, rec, Filter([Rule.udp() & Rule.port(53)]))
            rec_sel = eng.gather_rows(rec, 64, idx)          # records of the selected frames
            dns, tile_first, entries, total = eng.dns(sel, rec_sel)
            tunnels, inner = eng.decap(sel, rec_sel)
            dense = eng.gather(sel)                          # a packed batch of the selected bytes
        """
        torch = _torch()
        fc = flt.to_c()  # ValueError for what nexg_select_batch rejects
        rule = torch.empty(max(batch.count, 1), dtype=torch.uint8, device=self.torch_device) if want_rule else None
        idx, sel = self._compact(self.lib.nexg_select_batch, batch, abi.FRAMES_MONOTONE if _ordered(batch) else 0,
                                 before=(_frames(batch), _ptr(records), ctypes.byref(fc)), after=(_ptr(rule),),
                                 stream=stream)
        return (idx, sel, rule[: sel.count]) if want_rule else (idx, sel)

    @_on_stream
    def match(self, batch: FrameBatch, records, pset, stream=None):
        """Fixed-string match on frame bytes (nexg_match_batch; an extension,
        the reference has no payload search): which of up to 32 patterns of
        1..16 bytes occur in each frame's payload (or, with
        PatternSet(frame=True), anywhere in the frame), and where the first
        one starts. `records` is the uint8 device tensor a NEXG_OUT_RECORD
        parse of `batch` returned (None is valid with frame=True), `pset` a
        nex_amd.match.PatternSet. Returns a uint8 device tensor holding
        nexg_match[count] (abi.MATCH_DTYPE). One kernel, no synchronisation.

        The recipe: parse, match, narrow the table to the frames that carry
        what is looked for, compact the records, run the follow-up passes on
        those frames only, copy out just what matched:

            rec = eng.parse(batch, out_kind=abi.OUT_RECORD)
            rows = eng.match(batch, rec, PatternSet([Pattern(b"Host: ", nocase=True), Pattern.prefix(b"\\x16\\x03")]))
            idx, sel = eng.match_select(batch, rows, any=0b11)
            rec_sel = eng.gather_rows(rec, 64, idx)          # records of the selected frames
            dns, tile_first, entries, total = eng.dns(sel, rec_sel)
            dense = eng.gather(sel)                          # a packed batch of the selected bytes

        It composes with Engine.select through the tables: match the table
        select returned (with the gathered records), or select on the table
        match_select returned."""
        torch = _torch()
        pc = pset.to_c()  # ValueError for what nexg_match_batch rejects
        out = torch.empty(max(batch.count, 1) * 8, dtype=torch.uint8, device=self.torch_device)
        self._check(self.lib.nexg_match_batch(self.ctx, _frames(batch), _ptr(records), ctypes.byref(pc), _ptr(out),
                                              self._stream(stream)))
        return out[: batch.count * 8]

    @_on_stream
    def match_select(self, batch: FrameBatch, matches, any: int = 0, all: int = 0, none: int = 0,  # noqa: A002
                     stream=None):
        """Order-preserving selection by Engine.match's rows
        (nexg_match_select): frame i is selected when some bit of `any` is in
        its mask (any = 0: no such condition), every bit of `all` is, and no
        bit of `none` is; all three zero select every frame. Returns (index,
        selected) exactly as Engine.select returns them: index an int32
        device tensor (bit patterns of u32) with the frame number of each
        selected frame, selected a FrameBatch (offsets + lengths) over the
        same data whose count is the selected count. Allocates the workspace
        and reads the selected count back: one synchronisation of the stream."""
        for name, v in (("any", any), ("all", all), ("none", none)):
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise ValueError(f"{name} is a 32-bit mask")
        return self._compact(self.lib.nexg_match_select, batch, abi.FRAMES_MONOTONE if _ordered(batch) else 0,
                             before=(_frames(batch), _ptr(matches), int(any), int(all), int(none)), stream=stream)

    @_on_stream
    def gather(self, sel: FrameBatch, align: int = 1, stream=None):
        """Copy the frames of `sel` (usually Engine.select's table) into one
        dense buffer (nexg_gather_plan + nexg_gather_frames). Returns a new
        FrameBatch that owns its data: packed (offsets only) with align 1,
        offsets + lengths with each frame's start rounded up to `align`
        (4, 8 or 16) and the pads zero. A frame whose extent leaves the data
        or whose length exceeds 65535 is copied as length 0. Reads the total
        back: one synchronisation of the stream."""
        torch = _torch()
        if align not in abi.GATHER_ALIGNS:
            raise ValueError("align must be 1, 4, 8 or 16")
        dev = self.torch_device
        n = sel.count
        offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
        ln = torch.empty(max(n, 1), dtype=torch.int32, device=dev) if align != 1 else None
        ws_bytes = abi.gather_plan_workspace(n)
        ws = self._workspace(ws_bytes)
        fr = _frames(sel)
        s = self._stream(stream)
        self._check(self.lib.nexg_gather_plan(self.ctx, fr, align, _ptr(offs), _ptr(ln), _ptr(ws), ws_bytes, s))
        total = int(offs[n].item())  # waits for the kernels
        data = torch.empty(max(total, 16), dtype=torch.uint8, device=dev)
        self._check(self.lib.nexg_gather_frames(self.ctx, fr, _ptr(offs), _ptr(data), total, s))
        return FrameBatch(data=data[:total], count=n, offsets=offs, lengths=None if ln is None else ln[:n],
                          hints=0 if ln is None else abi.FRAMES_MONOTONE)

    @_on_stream
    def encap(self, batch: FrameBatch, tunnels, index=None, flows=None, align: int = 1, report=True, stream=None):
        """Every frame of `batch` copied into a new buffer behind an outer
        Ethernet / IP / UDP + VXLAN or GRE header (nexg_encap_plan +
        nexg_encap_frames): the bytes the reference's builders give around
        VxlanPacket::to_bytes / GrePacket::to_bytes. `tunnels` is a
        nex_amd.encap.TunnelSet, `index` a uint8 device tensor with one tunnel
        number per frame (abi.TUNNEL_NONE or any number past the set: the
        frame is copied unchanged) or None (tunnel 0 for every frame), `flows`
        the rows Engine.flow gave for the same table, needed when a spec
        takes its UDP source port from the flow hash. Returns (FrameBatch,
        rows): the batch owns its data, packed (offsets only) with align 1,
        offsets + lengths with each frame's start rounded up to `align` (4, 8
        or 16) and the pads zero; rows is the nexg_encapped[count] report
        (uint8 device tensor, abi.ENCAPPED_DTYPE) or None. A frame that
        cannot be wrapped (bad extent, too short for GRE_L3, outer frame over
        65535 bytes) has length 0 and its status in the row. Reads the total
        back: one synchronisation of the stream.

        The recipe, a tunnel endpoint as a match-action table: rule j of the
        filter gets tunnel j.

            rec = eng.parse(batch, out_kind=abi.OUT_RECORD)
            idx, sel, rule = eng.select(batch, rec, flt, want_rule=True)
            flows = eng.flow(sel, eng.gather_rows(rec, 64, idx))
            outer, rows = eng.encap(sel, tunnels, rule, flows)
        """
        torch = _torch()
        if align not in abi.GATHER_ALIGNS:
            raise ValueError("align must be 1, 4, 8 or 16")
        tc = tunnels.to_c()  # ValueError for what nexg_tunnels_check rejects
        if tunnels.needs_flows and flows is None:
            raise ValueError("a tunnel takes its source port from the flow hash: flows is needed")
        dev = self.torch_device
        n = batch.count
        if index is not None and (index.dtype != torch.uint8 or index.device != dev or index.numel() < n):
            raise ValueError(f"index: a uint8 tensor of {n} tunnel numbers on {dev} is needed")
        if flows is not None and (flows.device != dev or flows.numel() * flows.element_size() < n * 8):
            raise ValueError(f"flows: the {n} 8-byte rows of Engine.flow on {dev} are needed")
        offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
        ln = torch.empty(max(n, 1), dtype=torch.int32, device=dev) if align != 1 else None
        rows = torch.empty(max(n, 1) * 8, dtype=torch.uint8, device=dev) if report else None
        ws_bytes = abi.encap_plan_workspace(n)
        ws = self._workspace(ws_bytes)
        fr = _frames(batch)
        s = self._stream(stream)
        self._check(self.lib.nexg_encap_plan(self.ctx, fr, ctypes.byref(tc), _ptr(index), align, _ptr(offs), _ptr(ln),
                                             _ptr(ws), ws_bytes, s))
        total = int(offs[n].item())  # waits for the kernels
        data = torch.empty(max(total, 16), dtype=torch.uint8, device=dev)
        self._check(self.lib.nexg_encap_frames(self.ctx, fr, ctypes.byref(tc), _ptr(index), _ptr(flows), _ptr(offs),
                                               _ptr(data), total, _ptr(rows), s))
        out = FrameBatch(data=data[:total], count=n, offsets=offs, lengths=None if ln is None else ln[:n],
                         hints=0 if ln is None else abi.FRAMES_MONOTONE)
        return out, (rows[: n * 8] if report else None)

    @_on_stream
    def fragment(self, batch: FrameBatch, mtu: int, ignore_df: bool = False, align: int = 1, report=True, stream=None):
        """Every IPv4 frame of `batch` whose total length exceeds `mtu` (68 to
        65535) cut into RFC 791 fragments, every other frame copied unchanged
        (nexg_fragment_plan + nexg_fragment_frames; the rule is in
        include/nexg.h, restated by nex_amd.fragment.fragment_host). A frame
        with DF set that does not fit gives no output frame unless
        `ignore_df`, which clears DF in the pieces; nor does an IPv6 frame
        over the MTU, a bad extent or a fragment offset that would overflow:
        the row says which. Returns (FrameBatch, src_index, rows): the batch
        owns its data, packed (offsets only) with align 1, offsets + lengths
        with each output frame's start rounded up to `align` (4, 8 or 16) and
        the pads zero; src_index is an int32 device tensor (bit patterns of
        u32) with the input frame of each output frame, which
        Engine.gather_rows takes as it stands; rows is the
        nexg_fragged[count] report (uint8 device tensor, abi.FRAGGED_DTYPE)
        or None. Reads the two totals back: one synchronisation of the
        stream. ValueError when the output frames would number 2^32 - 1 or
        more (they are numbered with 32 bits).

        The recipe, a tunnel endpoint whose link has a 1500-byte MTU:

            outer, _ = eng.encap(sel, tunnels, rule, flows)
            pieces, src, rows = eng.fragment(outer, 1500)
            rule_of_piece = eng.gather_rows(rule_rows, 4, src)
        """
        torch = _torch()
        from .fragment import FragOption
        oc = FragOption(int(mtu), abi.FRAG_IGNORE_DF if ignore_df else 0, align).to_c()  # ValueError as the C check
        dev = self.torch_device
        n = batch.count
        first = torch.empty(n + 1, dtype=torch.int32, device=dev)
        nbytes = torch.empty(n + 1, dtype=torch.int64, device=dev)
        rows = torch.empty(max(n, 1) * 16, dtype=torch.uint8, device=dev) if report else None
        ws_bytes = abi.fragment_plan_workspace(n)
        ws = self._workspace(ws_bytes)
        fr = _frames(batch)
        s = self._stream(stream)
        self._check(self.lib.nexg_fragment_plan(self.ctx, fr, ctypes.byref(oc), _ptr(first), _ptr(nbytes), _ptr(rows),
                                                _ptr(ws), ws_bytes, s))
        totals = torch.stack((first[n].to(torch.int64) & 0xFFFFFFFF, nbytes[n])).cpu()  # waits for the kernels
        k, total = int(totals[0]), int(totals[1])
        if k == abi.FRAG_TOTAL_OVERFLOW:
            raise ValueError("2^32 - 1 output frames or more: fragment a part of the batch")
        offs = torch.empty(k + 1, dtype=torch.int64, device=dev)
        ln = torch.empty(max(k, 1), dtype=torch.int32, device=dev)
        src = torch.empty(max(k, 1), dtype=torch.int32, device=dev)
        data = torch.empty(max(total, 16), dtype=torch.uint8, device=dev)
        self._check(self.lib.nexg_fragment_frames(self.ctx, fr, ctypes.byref(oc), _ptr(first), _ptr(nbytes), k, _ptr(offs),
                                                  _ptr(ln), _ptr(src), _ptr(data), total, s))
        out = FrameBatch(data=data[:total], count=k, offsets=offs, lengths=None if align == 1 else ln[:k],
                         hints=0 if align == 1 else abi.FRAMES_MONOTONE)
        return out, src[:k], (rows[: n * 16] if report else None)

    @_on_stream
    def gather_rows(self, rows, row_bytes: int, index, stream=None):
        """Compact per-frame rows by a selected index (nexg_gather_rows):
        row k of the result is rows[index[k]], zeros where index[k] is past
        the rows. `rows` is a device tensor of whole rows of `row_bytes` (4,
        8, 16, 32 or 64: flags words, descriptors, nexg_tunnel, nexg_dns,
        records), `index` the int32 tensor Engine.select returned. Returns a
        uint8 device tensor of len(index) * row_bytes bytes."""
        torch = _torch()
        if row_bytes not in abi.GATHER_ROW_BYTES:
            raise ValueError("row_bytes must be 4, 8, 16, 32 or 64")
        n = index.numel()
        rows_count = rows.numel() * rows.element_size() // row_bytes
        out = torch.empty(max(n, 1) * row_bytes, dtype=torch.uint8, device=self.torch_device)
        self._check(self.lib.nexg_gather_rows(self.ctx, _ptr(rows), row_bytes, rows_count, _ptr(index), n, _ptr(out),
                                              self._stream(stream)))
        return out[: n * row_bytes]

    @_on_stream
    def flow(self, batch: FrameBatch, records, option=None, stream=None):
        """A flow row per frame (nexg_flow_batch; an extension, the reference
        has no flow notion): the Toeplitz RSS hash of the frame's addresses
        and ports as NICs compute it, with the kind of key, the IP protocol
        and whether FlowOption(symmetric=True) exchanged the endpoints.
        `records` is the uint8 device tensor a NEXG_OUT_RECORD parse of
        `batch` returned (for an inner table from Engine.decap: the inner
        records), `option` a nex_amd.flow.FlowOption. Returns a uint8 device
        tensor holding nexg_flow[count] (abi.FLOW_DTYPE); frames without an
        IP layer or with an error status have an all-zero row.

        The recipe for handing each flow to one worker:

            rec = eng.parse(batch, out_kind=abi.OUT_RECORD)
            flows = eng.flow(batch, rec, FlowOption(symmetric=True))
            index, table, first = eng.flow_partition(batch, flows, 8)
            rec_by_bucket = eng.gather_rows(rec, 64, index)
            for b in range(8):
                part = eng.flow_bucket(table, first, b)      # a FrameBatch view, no copy
                rec_b = rec_by_bucket[first[b] * 64: first[b + 1] * 64]
        """
        from .flow import FlowOption
        torch = _torch()
        fo = (option if option is not None else FlowOption()).to_c()  # ValueError for what nexg_flow_batch rejects
        out = torch.empty(max(batch.count, 1) * 8, dtype=torch.uint8, device=self.torch_device)
        self._check(self.lib.nexg_flow_batch(self.ctx, _frames(batch), _ptr(records), ctypes.byref(fo), _ptr(out),
                                             self._stream(stream)))
        return out[: batch.count * 8]

    @_on_stream
    def flow_partition(self, batch: FrameBatch, flows, buckets: int, stream=None):
        """Stable split of `batch` into `buckets` (1..256) buckets by
        flows[i].hash % buckets (nexg_flow_partition): every flow lands whole
        in one bucket, frames keep their order inside a bucket, frames without
        a flow go to bucket 0. `flows` is the tensor Engine.flow returned.
        Returns (index, table, bucket_first): index an int32 device tensor
        (bit patterns of u32) with the frame number of each output entry,
        table a FrameBatch (offsets + lengths) of `count` frames in bucket
        order over the same data, bucket_first a host int64 array of
        buckets + 1 entries (bucket b is entries bucket_first[b] to
        bucket_first[b + 1]; Engine.flow_bucket gives it as a batch).
        Engine.gather_rows with index reorders records or any other per-frame
        rows to match. Allocates the workspace and reads bucket_first back:
        one synchronisation of the stream."""
        torch = _torch()
        if not 1 <= int(buckets) <= abi.FLOW_MAX_BUCKETS:
            raise ValueError("buckets must be 1..256")
        count = batch.count
        idx, off, ln = self._table(count)
        first = torch.empty(buckets + 1, dtype=torch.int64, device=self.torch_device)
        ws_bytes = abi.flow_partition_workspace(count, buckets)
        ws = self._workspace(ws_bytes)
        self._check(self.lib.nexg_flow_partition(self.ctx, _frames(batch), _ptr(flows), int(buckets), _ptr(idx),
                                                 _ptr(off), _ptr(ln), _ptr(first), _ptr(ws), ws_bytes,
                                                 self._stream(stream)))
        host_first = first.cpu().numpy()  # waits for the kernels
        ordered = _ordered(batch)
        # monotone inside each bucket (Engine.flow_bucket's views), not across bucket boundaries
        table = FrameBatch(data=batch.data, count=count, offsets=off[:count], lengths=ln[:count],
                           hints=abi.FRAMES_MONOTONE if ordered and buckets == 1 else 0,
                           bucket_hints=abi.FRAMES_MONOTONE if ordered else 0)
        return idx[:count], table, host_first

    @staticmethod
    def flow_bucket(table: FrameBatch, bucket_first, b: int) -> FrameBatch:
        """Bucket `b` of Engine.flow_partition's table as a FrameBatch view
        over the same data and the same offset / length tensors (nothing is
        copied), ready for parse, decap, dns, select and gather."""
        lo, hi = int(bucket_first[b]), int(bucket_first[b + 1])
        return FrameBatch(data=table.data, count=hi - lo, offsets=table.offsets[lo:hi], lengths=table.lengths[lo:hi],
                          hints=table.bucket_hints | table.hints)

    @_on_stream
    def flow_sort(self, flows, stream=None):
        """The frame numbers of a batch ordered by (flows[i].hash ascending,
        frame number ascending) (nexg_flow_sort): a stable radix sort on the
        device, so every flow is one contiguous run and frames without a flow
        (hash 0) come first. `flows` is the tensor Engine.flow returned.
        Returns an int32 device tensor (bit patterns of u32) of `count`
        entries. Allocates the workspace; no synchronisation."""
        torch = _torch()
        count = flows.numel() * flows.element_size() // 8
        idx = torch.empty(max(count, 1), dtype=torch.int32, device=self.torch_device)
        ws_bytes = abi.flow_sort_workspace(count)
        ws = self._workspace(ws_bytes)
        self._check(self.lib.nexg_flow_sort(self.ctx, _ptr(flows), count, _ptr(idx), _ptr(ws), ws_bytes,
                                            self._stream(stream)))
        return idx[:count]

    @_on_stream
    def flow_groups(self, batch: FrameBatch, records, flows, option=None, order=None, groups_cap=None, stream=None):
        """Per-flow counters of a batch (nexg_flow_groups): one row per run of
        equal hashes in the sorted order, with its packets, its bytes, its
        first frame and `mixed`, the number of members whose flow key differs
        from the member before them (nonzero only where two flows share one
        32-bit hash; the members order[first: first + packets] tell them
        apart). `records` and `flows` are the tensors Engine.parse
        (NEXG_OUT_RECORD) and Engine.flow returned for `batch`, `option` the
        FlowOption given to Engine.flow, `order` Engine.flow_sort's tensor
        (None: sorted here). Returns (groups, group_of, n_groups, order):
        groups a uint8 device tensor holding nexg_flow_group[n_groups]
        (abi.FLOW_GROUP_DTYPE), group_of an int32 device tensor with the group
        number of every frame, n_groups an int. The rows are sized by reading
        the group count back (one synchronisation of the stream) and the pass
        runs once more to fill them; with `groups_cap` given it runs once,
        rows at or past the capacity are not stored, and n_groups may exceed it.

        The recipe for a flow table of one batch:

            rec = eng.parse(batch, out_kind=abi.OUT_RECORD)
            flows = eng.flow(batch, rec, FlowOption(symmetric=True))
            groups, group_of, n, order = eng.flow_groups(batch, rec, flows, FlowOption(symmetric=True))
            first_index = groups.view(torch.int32).view(-1, 8)[:, 7]
            first_rec = eng.gather_rows(rec, 64, first_index)     # each flow's first record
        """
        from .flow import FlowOption
        torch = _torch()
        fo = (option if option is not None else FlowOption()).to_c()  # ValueError for what nexg_flow_groups rejects
        count = batch.count
        dev = self.torch_device
        if order is None:
            order = self.flow_sort(flows, stream)
        group_of = torch.empty(max(count, 1), dtype=torch.int32, device=dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        ws_bytes = abi.flow_groups_workspace(count)
        ws = self._workspace(ws_bytes)
        fr = _frames(batch)
        s = self._stream(stream)

        def run(rows, cap, gof):
            self._check(self.lib.nexg_flow_groups(self.ctx, fr, _ptr(records), _ptr(flows), ctypes.byref(fo),
                                                  _ptr(order), _ptr(rows), cap, _ptr(gof), _ptr(cnt), _ptr(ws), ws_bytes, s))

        if groups_cap is not None:
            cap = int(groups_cap)
            groups = torch.empty(max(cap, 1) * 32, dtype=torch.uint8, device=dev)
            run(groups, cap, group_of)
            n = int(cnt.item())  # waits for the kernels
            return groups[: min(n, cap) * 32], group_of[:count], n, order
        run(None, 0, group_of)  # the count and the group numbers
        n = int(cnt.item())  # waits for the kernels
        groups = torch.empty(max(n, 1) * 32, dtype=torch.uint8, device=dev)
        if n:
            run(groups, n, None)
        return groups[: n * 32], group_of[:count], n, order

    @_on_stream
    def flow_table_merge(self, batch: FrameBatch, records, groups, table=None, epoch=0, min_epoch=0, option=None,
                         table_cap=None, out=None, stream=None):
        """Merge one batch's groups into a flow table (nexg_flow_table_merge):
        the union by hash of `table` and `groups`, ascending. `groups` is the
        uint8 device tensor Engine.flow_groups returned for `batch` (whole
        nexg_flow_group rows), `records` the batch's records, `option` the
        FlowOption given to Engine.flow, `table` a uint8 device tensor holding
        nexg_flow_entry rows (abi.FLOW_ENTRY_DTYPE) ascending by hash, or
        None for an empty table; it is not changed. A hash in both adds the
        group's packets and bytes to the entry and sets last_epoch = epoch; a
        new hash makes an entry; an entry no group matches is dropped when
        last_epoch < min_epoch. MIXED (flags8 bit 0) marks an entry under
        which more than one flow key has been counted.

        Returns (table_out, n_out, slot): the new table as a uint8 device
        tensor of min(n_out, table_cap) entries, written into `out` when
        given (a uint8 device tensor of table_cap entries that does not
        overlap `table`), n_out the size of the union (an int: one
        synchronisation of the stream; it may exceed table_cap, whose default
        is room for every entry and group), slot an int32 device tensor with
        the position in the union of every group's entry."""
        from .flow import FlowOption
        torch = _torch()
        fo = (option if option is not None else FlowOption()).to_c()  # ValueError for what the merge rejects
        dev = self.torch_device
        n_groups = groups.numel() * groups.element_size() // 32
        n_in = 0 if table is None else table.numel() * table.element_size() // 64
        cap = n_in + n_groups if table_cap is None else int(table_cap)
        if out is None:
            out = torch.empty(max(cap, 1) * 64, dtype=torch.uint8, device=dev)
        elif out.numel() * out.element_size() < cap * 64:
            raise ValueError(f"out holds {out.numel() * out.element_size()} B; {cap} entries need {cap * 64} B")
        slot = torch.empty(max(n_groups, 1), dtype=torch.int32, device=dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        ws_bytes = abi.flow_table_workspace(n_in, n_groups)
        ws = self._workspace(ws_bytes)
        self._check(self.lib.nexg_flow_table_merge(self.ctx, _frames(batch), _ptr(records), ctypes.byref(fo),
                                                   _ptr(groups) if n_groups else None, n_groups,
                                                   _ptr(table) if n_in else None, n_in, int(epoch), int(min_epoch),
                                                   _ptr(out), cap, _ptr(slot), _ptr(cnt), _ptr(ws), ws_bytes,
                                                   self._stream(stream)))
        n_out = int(cnt.item())  # waits for the kernels
        return out[: min(n_out, cap) * 64], n_out, slot[:n_groups]

    @_on_stream
    def dns(self, batch: FrameBatch, records, port: int = abi.DNS_PORT, any_udp: bool = False, entries_cap=None,
            stream=None):
        """Walk every DNS message of `batch` in place (nexg_dns_batch +
        nexg_dns_entries; DnsPacket::try_from_buf dns.rs:1166-1259 on
        Frame.payload). `records` is the uint8 device tensor a NEXG_OUT_RECORD
        parse of `batch` returned. A frame is tried when it is UDP with a
        non-empty payload from or to `port` (any_udp: every such UDP frame,
        as dns_dump.rs:98-100 does).

        Returns (dns, tile_first, entries, total): uint8 device tensors
        holding nexg_dns[count] (abi.DNS_DTYPE) and nexg_dns_entry rows
        (abi.DNS_ENTRY_DTYPE), tile_first an int64 device tensor of
        ceil(count / 256) + 1 prefix sums. The k-th entry of frame i is row
        tile_first[i >> 8] + dns[i].first + k (nex_amd.dns.frame_entries).

        entries_cap=None reads the total back (one synchronisation of the
        stream), allocates exactly that many rows and fills them; total is
        then an int. With a capacity given both calls are enqueued without a
        synchronisation, rows at or past the capacity are not written, and
        total is the one-element device tensor tile_first[-1:]."""
        torch = _torch()
        n = batch.count
        dev = self.torch_device
        out = torch.empty(max(n, 1) * 32, dtype=torch.uint8, device=dev)
        tile_first = torch.empty(abi.dns_tile_first_bytes(n) // 8, dtype=torch.int64, device=dev)
        fr = _frames(batch)
        opt = abi.DnsOption(abi.DNS_ANY_UDP if any_udp else 0, port, 0)
        s = self._stream(stream)
        self._check(self.lib.nexg_dns_batch(self.ctx, fr, _ptr(records), ctypes.byref(opt), _ptr(out),
                                            _ptr(tile_first), s))
        if entries_cap is None:
            total = cap = int(tile_first[-1].item())  # waits for the kernels
        else:
            total, cap = tile_first[-1:], int(entries_cap)
        entries = torch.empty(max(cap, 1) * 16, dtype=torch.uint8, device=dev)
        self._check(self.lib.nexg_dns_entries(self.ctx, fr, _ptr(out), _ptr(tile_first), _ptr(entries), cap, s))
        return out[: n * 32], tile_first, entries[: cap * 16], total

    @_on_stream
    def probe_stream(self, data, write8, out=None, stream=None):
        """Calibration stream over a uint8 device tensor (nexg_probe_stream):
        the parse kernels' load shape, read-only or with the 8-B-per-64-B
        descriptor store stream (write8 = 9: that stream at the fixed-stride
        parse kernel's 6 workgroups per CU). Not a reference entry point."""
        torch = _torch()
        nbytes = data.numel() // 16384 * 16384
        if out is None:
            n = nbytes // 64 * 8 if write8 else nbytes // 16384 * 4
            out = torch.empty(max(n, 8), dtype=torch.uint8, device=self.torch_device)
        self._check(self.lib.nexg_probe_stream(self.ctx, _ptr(data), nbytes, 9 if write8 == 9 else 8 if write8 else 0,
                                               _ptr(out), self._stream(stream)))
        return out

    @_on_stream
    def probe_write(self, out, stream=None):
        """Write-only calibration stream (nexg_probe_stream, out_per_64 = 64):
        the builders' copy-out shape over a uint8 device tensor (whole 16-KiB
        tiles). Not a reference entry point."""
        nbytes = out.numel() // 16384 * 16384
        self._check(self.lib.nexg_probe_stream(self.ctx, None, nbytes, 64, _ptr(out), self._stream(stream)))
        return out

    @_on_stream
    def probe_span_clock(self, batch: FrameBatch, option: ParseOption = ParseOption(),
                         mode: ParseMode = ParseMode.Lenient, out=None, stream=None):
        """One stamped launch of the span kernel over `batch`
        (nexg_probe_span_clock; calibration, not a reference entry point):
        returns (grouped output, stamps) device tensors, stamps int64
        (workgroups, 8) as include/nexg.h lays them out; span_clock_summary
        reduces them on the host."""
        torch = _torch()
        nbytes = self.out_bytes(abi.OUT_GROUPED, batch.count)
        if out is None:
            out = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self.torch_device)
        nwg = max(1, (batch.count + 255) // 256)
        stamps = torch.zeros((nwg, 8), dtype=torch.int64, device=self.torch_device)
        opt = abi.ParseOptionC(option.flags(mode), option.offset)
        self._check(self.lib.nexg_probe_span_clock(self.ctx, _frames(batch), ctypes.byref(opt), _ptr(out),
                                                   _ptr(stamps), self._stream(stream)))
        return out, stamps

    @_on_stream
    def probe_latency(self, buf, steps: int = 2000, start: int = 0, loaded: bool = False, stream=None):
        """Dependent HBM load latency (nexg_probe_latency; calibration, not a
        reference entry point) over a uint8 device scratch tensor (>= 4 MiB):
        returns (ns per step, shader-clock cycles per step)."""
        torch = _torch()
        out = torch.zeros(4, dtype=torch.int64, device=self.torch_device)
        nbytes = buf.numel() // 64 * 64
        self._check(self.lib.nexg_probe_latency(self.ctx, _ptr(buf), nbytes, int(steps), int(start) & 0xFFFFFFFF,
                                                1 if loaded else 0, _ptr(out), self._stream(stream)))
        torch.cuda.synchronize(self.torch_device)
        cyc, ticks = (int(v) for v in out[:2].cpu())
        return ticks * 10.0 / steps, cyc / steps

    @_on_stream
    def checksum(self, batch: FrameBatch, skipword: int, stream=None):
        """util::checksum(buf, skipword) per buffer (util.rs:65)."""
        torch = _torch()
        out = torch.empty(max(batch.count, 1), dtype=torch.int16, device=self.torch_device)
        skip = min(int(skipword), 0xFFFFFFFF)
        self._check(self.lib.nexg_checksum_batch(self.ctx, _frames(batch), skip, _ptr(out),
                                                 self._stream(stream)))
        return out[: batch.count]

    # --- serialize path ---------------------------------------------------
    @staticmethod
    def _check_rows(count, row_bytes, shared_ok=False, **arrays):
        """Per-frame parameter arrays hold `count` rows of `row_bytes` each
        (or exactly one row where the builder takes one value for the batch,
        `shared_ok`): the kernels read row i for frame i, so a short array
        would be read past on the device."""
        for name, t in arrays.items():
            if t is None:
                continue
            nb = t.numel() * t.element_size()
            if shared_ok and nb == row_bytes:
                continue
            if nb < count * row_bytes:
                raise ValueError(f"{name} holds {nb} B; {count} frames need {count * row_bytes} B"
                                 + (f" (or one {row_bytes}-B value for the batch)" if shared_ok else ""))

    @staticmethod
    def _check_out(out, count, stride):
        if out is not None and out.numel() * out.element_size() < count * stride:
            raise ValueError(f"out holds {out.numel() * out.element_size()} B; {count} frames of stride "
                             f"{stride} need {count * stride} B")

    @_on_stream
    def build_udp4(self, src_ip, dst_ip, src_port=None, dst_port=None, ip_id=None,
                   def_src_port=0, def_dst_port=0, def_ip_id=0,
                   src_mac=b"\0" * 6, dst_mac=b"\0" * 6, ttl=64, ip_flags=0, dscp_ecn=0,
                   payload=None, out_stride=None, out=None, stream=None, def_src_ip=0):
        """UdpPacketBuilder -> Ipv4PacketBuilder -> EthernetPacketBuilder
        (udp_ping.rs:68-109) on every tuple. Tensors are int32/int16 device
        tensors holding the u32/u16 values; src_ip=None takes def_src_ip (a
        u32 value) for every frame — with no other array, the udp_ping probe
        batch: one source, one port pair, a destination per frame."""
        torch = _torch()
        count = dst_ip.numel()
        plen = 0 if payload is None else payload.numel()
        stride = out_stride or (42 + plen)
        self._check_rows(count, 4, src_ip=src_ip)
        self._check_rows(count, 2, src_port=src_port, dst_port=dst_port, ip_id=ip_id)
        self._check_out(out, count, stride)
        if out is None:
            out = torch.empty(max(count, 1) * stride, dtype=torch.uint8, device=self.torch_device)
        p = abi.Udp4Build()
        p.src_ip = None if src_ip is None else src_ip.data_ptr()
        p.dst_ip = dst_ip.data_ptr()
        p.def_src_ip = def_src_ip & 0xFFFFFFFF
        p.src_port = None if src_port is None else src_port.data_ptr()
        p.dst_port = None if dst_port is None else dst_port.data_ptr()
        p.ip_id = None if ip_id is None else ip_id.data_ptr()
        p.src_mac = p.dst_mac = None
        p.payload = None if payload is None else payload.data_ptr()
        p.payload_len = plen
        p.def_src_port, p.def_dst_port, p.def_ip_id = def_src_port, def_dst_port, def_ip_id
        p.def_src_mac[:] = list(src_mac)
        p.def_dst_mac[:] = list(dst_mac)
        p.ttl, p.ip_flags, p.dscp_ecn, p.count = ttl, ip_flags, dscp_ecn, count
        self._check(self.lib.nexg_build_udp4_batch(self.ctx, ctypes.byref(p), _ptr(out), stride,
                                                   self._stream(stream)))
        return out

    @staticmethod
    def pack_udp4_tuples(src_ip, dst_ip, src_port, dst_port, ip_id):
        """The five per-frame tuple arrays of build_udp4 (int32 / int16 device
        tensors) as one (count, 4) int32 tensor of 16-B nexg_udp4_tuple records."""
        torch = _torch()
        lo16 = lambda t: t.to(torch.int32) & 0xFFFF
        return torch.stack([src_ip.to(torch.int32), dst_ip.to(torch.int32),
                            lo16(src_port) | (lo16(dst_port) << 16), lo16(ip_id)], dim=1).contiguous()

    @_on_stream
    def build_udp4_tuples(self, tuples, src_mac=b"\0" * 6, dst_mac=b"\0" * 6, ttl=64, ip_flags=0, dscp_ecn=0,
                          payload=None, out_stride=None, out=None, stream=None):
        """build_udp4 with each frame's tuple as one 16-B record
        (nexg_build_udp4_tuples; `tuples` from pack_udp4_tuples)."""
        torch = _torch()
        count = tuples.shape[0]
        plen = 0 if payload is None else payload.numel()
        stride = out_stride or (42 + plen)
        self._check_rows(count, 16, tuples=tuples)
        self._check_out(out, count, stride)
        if out is None:
            out = torch.empty(max(count, 1) * stride, dtype=torch.uint8, device=self.torch_device)
        p = abi.Udp4Build()
        p.payload = None if payload is None else payload.data_ptr()
        p.payload_len = plen
        p.def_src_mac[:] = list(src_mac)
        p.def_dst_mac[:] = list(dst_mac)
        p.ttl, p.ip_flags, p.dscp_ecn, p.count = ttl, ip_flags, dscp_ecn, count
        self._check(self.lib.nexg_build_udp4_tuples(self.ctx, ctypes.byref(p), _ptr(tuples), _ptr(out), stride,
                                                    self._stream(stream)))
        return out

    @_on_stream
    def build_udp6(self, src_ip, dst_ip, src_port=None, dst_port=None, def_src_port=0,
                   def_dst_port=0, src_mac=b"\0" * 6, dst_mac=b"\0" * 6, hop_limit=64,
                   traffic_class=0, flow_label=0, payload=None, out_stride=None, out=None,
                   stream=None):
        """udp_ping's IPv6 branch (udp_ping.rs:83-89): UdpPacketBuilder ->
        Ipv6PacketBuilder -> EthernetPacketBuilder on every tuple. src_ip /
        dst_ip are (count, 16) uint8 device tensors in network order; src_ip
        may be one address (every frame's source: the probe batch)."""
        torch = _torch()
        count = dst_ip.shape[0] if dst_ip.dim() > 1 else dst_ip.numel() // 16
        plen = 0 if payload is None else payload.numel()
        stride = out_stride or (62 + plen)
        self._check_rows(count, 16, shared_ok=True, src_ip=src_ip)
        self._check_rows(count, 2, src_port=src_port, dst_port=dst_port)
        self._check_out(out, count, stride)
        if out is None:
            out = torch.empty(max(count, 1) * stride, dtype=torch.uint8, device=self.torch_device)
        p = abi.Udp6Build()
        p.src_ip, p.dst_ip = src_ip.data_ptr(), dst_ip.data_ptr()
        p.src_shared = 1 if src_ip.numel() == 16 and count != 1 else 0
        p.src_port = None if src_port is None else src_port.data_ptr()
        p.dst_port = None if dst_port is None else dst_port.data_ptr()
        p.src_mac = p.dst_mac = None
        p.payload = None if payload is None else payload.data_ptr()
        p.payload_len = plen
        p.flow_label = flow_label
        p.def_src_port, p.def_dst_port = def_src_port, def_dst_port
        p.def_src_mac[:] = list(src_mac)
        p.def_dst_mac[:] = list(dst_mac)
        p.hop_limit, p.traffic_class, p.count = hop_limit, traffic_class, count
        self._check(self.lib.nexg_build_udp6_batch(self.ctx, ctypes.byref(p), _ptr(out), stride,
                                                   self._stream(stream)))
        return out

    @staticmethod
    def _ip_build(family, src_ip, dst_ip, ip_id, def_ip_id, src_mac, dst_mac, ttl, ip_flags, tos,
                  flow_label):
        """src_ip: (count, 4|16) per frame, or ONE address ((4|16,) or (1, 4|16)):
        the probe batches' single source (nexg_ip_build.src_shared)."""
        ip = abi.IpBuild()
        ip.src_ip, ip.dst_ip = src_ip.data_ptr(), dst_ip.data_ptr()
        w = 4 if family == 4 else 16
        ip.src_shared = 1 if src_ip.numel() == w and dst_ip.numel() != w else 0
        ip.ip_id = None if ip_id is None else ip_id.data_ptr()
        ip.src_mac = ip.dst_mac = None
        ip.family, ip.flow_label, ip.def_ip_id = family, flow_label, def_ip_id
        ip.def_src_mac[:] = list(src_mac)
        ip.def_dst_mac[:] = list(dst_mac)
        ip.ttl, ip.ip_flags, ip.tos = ttl, ip_flags, tos
        return ip

    @_on_stream
    def build_tcp(self, family, src_ip, dst_ip, src_port=None, dst_port=None, seq=None, ack=None,
                  def_src_port=0, def_dst_port=0, def_seq=0, def_ack=0, flags=0, window=0xFFFF,
                  urgent_ptr=0, options=b"", payload=None, ip_id=None, def_ip_id=0,
                  src_mac=b"\0" * 6, dst_mac=b"\0" * 6, ttl=64, ip_flags=0, tos=0, flow_label=0,
                  out_stride=None, out=None, stream=None):
        """tcp_ping (examples/tcp_ping.rs:111-163): TcpPacketBuilder -> IPv4/IPv6
        builder -> EthernetPacketBuilder on every tuple. Addresses are
        (count, 4|16) uint8 device tensors (src_ip may be one address: every
        frame's source); ports/ids int16, seq/ack int32. One source, a
        destination per frame and no other array is tcp_ping's probe batch."""
        torch = _torch()
        count = dst_ip.shape[0]
        plen = 0 if payload is None else payload.numel()
        padded = (len(options) + 3) // 4 * 4
        flen = 14 + (20 if family == 4 else 40) + 20 + padded + plen
        stride = out_stride or flen
        w = 4 if family == 4 else 16
        self._check_rows(count, w, shared_ok=True, src_ip=src_ip)
        self._check_rows(count, 2, src_port=src_port, dst_port=dst_port, ip_id=ip_id)
        self._check_rows(count, 4, seq=seq, ack=ack)
        self._check_out(out, count, stride)
        if out is None:
            out = torch.empty(max(count, 1) * stride, dtype=torch.uint8, device=self.torch_device)
        p = abi.TcpBuild()
        p.ip = self._ip_build(family, src_ip, dst_ip, ip_id, def_ip_id, src_mac, dst_mac, ttl,
                              ip_flags, tos, flow_label)
        p.src_port = None if src_port is None else src_port.data_ptr()
        p.dst_port = None if dst_port is None else dst_port.data_ptr()
        p.seq = None if seq is None else seq.data_ptr()
        p.ack = None if ack is None else ack.data_ptr()
        p.payload = None if payload is None else payload.data_ptr()
        p.payload_len = plen
        p.def_seq, p.def_ack, p.def_src_port, p.def_dst_port = def_seq, def_ack, def_src_port, def_dst_port
        p.window, p.urgent_ptr, p.flags = window, urgent_ptr, flags
        p.options_len = min(len(options), 255)
        p.options[:min(len(options), 40)] = list(options[:40])
        p.count = count
        self._check(self.lib.nexg_build_tcp_batch(self.ctx, ctypes.byref(p), _ptr(out), stride,
                                                  self._stream(stream)))
        return out

    @_on_stream
    def build_icmp_echo(self, family, src_ip, dst_ip, identifier=None, sequence=None,
                        def_identifier=0, def_sequence=0, icmp_type=None, icmp_code=0, payload=None,
                        ip_id=None, def_ip_id=0, src_mac=b"\0" * 6, dst_mac=b"\0" * 6, ttl=64,
                        ip_flags=0, tos=0, flow_label=0, out_stride=None, out=None, stream=None):
        """icmp_ping (examples/icmp_ping.rs:67-102): Icmp(v6)PacketBuilder with
        echo_fields -> IPv4/IPv6 builder -> EthernetPacketBuilder. src_ip may
        be one address (every frame's source: icmp_ping's probe batch)."""
        torch = _torch()
        count = dst_ip.shape[0]
        plen = 0 if payload is None else payload.numel()
        flen = 14 + (20 if family == 4 else 40) + 8 + plen
        stride = out_stride or flen
        w = 4 if family == 4 else 16
        self._check_rows(count, w, shared_ok=True, src_ip=src_ip)
        self._check_rows(count, 2, identifier=identifier, sequence=sequence, ip_id=ip_id)
        self._check_out(out, count, stride)
        if out is None:
            out = torch.empty(max(count, 1) * stride, dtype=torch.uint8, device=self.torch_device)
        p = abi.IcmpEchoBuild()
        p.ip = self._ip_build(family, src_ip, dst_ip, ip_id, def_ip_id, src_mac, dst_mac, ttl,
                              ip_flags, tos, flow_label)
        p.identifier = None if identifier is None else identifier.data_ptr()
        p.sequence = None if sequence is None else sequence.data_ptr()
        p.payload = None if payload is None else payload.data_ptr()
        p.payload_len = plen
        p.def_identifier, p.def_sequence = def_identifier, def_sequence
        p.icmp_type = (8 if family == 4 else 128) if icmp_type is None else icmp_type
        p.icmp_code = icmp_code
        p.count = count
        self._check(self.lib.nexg_build_icmp_echo_batch(self.ctx, ctypes.byref(p), _ptr(out), stride,
                                                        self._stream(stream)))
        return out

    # --- synthetic workloads ----------------------------------------------
    @_on_stream
    def build_arp(self, target_ip, sender_ip=None, def_sender_ip=b"\0" * 4, sender_mac=None,
                  def_sender_mac=b"\0" * 6, target_mac=None, def_target_mac=b"\0" * 6, eth_dst=None,
                  def_eth_dst=b"\xff" * 6, hardware_type=1, protocol_type=0x0800, operation=1,
                  hw_addr_len=6, proto_addr_len=4, out_stride=42, out=None, stream=None):
        """examples/arp.rs:59-67: ArpPacketBuilder::new(sender_mac, sender_ip,
        target_ip) (builder/arp.rs) behind EthernetPacketBuilder (broadcast
        destination) on every target. Addresses are (count, 4) / (count, 6)
        uint8 device tensors or None for the defaults."""
        torch = _torch()
        count = target_ip.shape[0]
        if out is None:
            out = torch.empty(max(count, 1) * out_stride, dtype=torch.uint8, device=self.torch_device)
        p = abi.ArpBuild()
        p.target_ip = target_ip.data_ptr()
        p.sender_ip = None if sender_ip is None else sender_ip.data_ptr()
        p.sender_mac = None if sender_mac is None else sender_mac.data_ptr()
        p.target_mac = None if target_mac is None else target_mac.data_ptr()
        p.eth_dst = None if eth_dst is None else eth_dst.data_ptr()
        p.def_sender_ip[:] = list(def_sender_ip)
        p.def_sender_mac[:] = list(def_sender_mac)
        p.def_target_mac[:] = list(def_target_mac)
        p.def_eth_dst[:] = list(def_eth_dst)
        p.hardware_type, p.protocol_type, p.operation = hardware_type, protocol_type, operation
        p.hw_addr_len, p.proto_addr_len = hw_addr_len, proto_addr_len
        p.count = count
        self._check(self.lib.nexg_build_arp_batch(self.ctx, ctypes.byref(p), _ptr(out), out_stride,
                                                  self._stream(stream)))
        return out

    @_on_stream
    def build_ndp_ns(self, src_ip, target_ip, src_mac=b"\0" * 6, dst_mac=None, hop_limit=255, tos=0,
                     flow_label=0, out_stride=86, out=None, stream=None):
        """examples/ndp.rs:82-108: NdpPacketBuilder::new(src_mac, src_ip,
        target) (builder/ndp.rs) -> Ipv6PacketBuilder (next header 58, hop
        limit 255) -> EthernetPacketBuilder with destination 33:33 + the
        target's last four bytes (ipv6_multicast_mac), or `dst_mac` when
        given. Addresses are (count, 16) uint8 device tensors."""
        torch = _torch()
        count = target_ip.shape[0]
        if out is None:
            out = torch.empty(max(count, 1) * out_stride, dtype=torch.uint8, device=self.torch_device)
        p = abi.NdpNsBuild()
        p.ip = self._ip_build(6, src_ip, target_ip, None, 0, src_mac, dst_mac or b"\0" * 6, hop_limit, 0, tos,
                              flow_label)
        p.eth_dst_multicast = 1 if dst_mac is None else 0
        p.count = count
        self._check(self.lib.nexg_build_ndp_ns_batch(self.ctx, ctypes.byref(p), _ptr(out), out_stride,
                                                     self._stream(stream)))
        return out

    @_on_stream
    def gen_batch(self, workload: int, count: int, seed: int = abi.DEFAULT_SEED,
                  first_index: int = 0, stream=None, record_gap: int = 0) -> FrameBatch:
        """Device-generated SURVEY.md App. C workload (UDP64: fixed 64-B
        stride; IMIX: packed with an int64 offset table of count+1 entries).
        record_gap > 0 (IMIX): each frame preceded by that many zero bytes and
        described by offsets + lengths + the monotone hint, the shape
        nexg_pcap_read_raw hands over (16 = classic pcap record headers)."""
        torch = _torch()
        dev = self.torch_device
        s = self._stream(stream)
        if workload == abi.WL_UDP64:
            data = torch.empty(max(count, 1) * 64, dtype=torch.uint8, device=dev)
            self._check(self.lib.nexg_gen_frames(self.ctx, workload, seed, first_index, count,
                                                 _ptr(data), None, 64, s))
            return FrameBatch(data=data, count=count, stride=64)
        lengths = torch.empty(max(count, 1), dtype=torch.int32, device=dev)
        self._check(self.lib.nexg_gen_lengths(self.ctx, workload, seed, first_index, count,
                                              _ptr(lengths), s))
        offsets = torch.zeros(count + 1, dtype=torch.int64, device=dev)
        if count:
            torch.cumsum(lengths[:count].to(torch.int64) + record_gap, 0, out=offsets[1:])
        total = int(offsets[count].item()) if count else 0
        if record_gap:
            offsets = offsets + record_gap  # frame i starts after its record header
            data = torch.zeros(max(total, 16) + 16, dtype=torch.uint8, device=dev)
        else:
            data = torch.empty(max(total, 16) + 16, dtype=torch.uint8, device=dev)
        self._check(self.lib.nexg_gen_frames(self.ctx, workload, seed, first_index, count,
                                             _ptr(data), _ptr(offsets), 0, s))
        if record_gap:
            return FrameBatch(data=data[:max(total, 16)], count=count, offsets=offsets,
                              lengths=lengths, hints=abi.FRAMES_MONOTONE)
        return FrameBatch(data=data, count=count, offsets=offsets)

    @_on_stream
    def gen_udp4_params(self, count, seed=abi.DEFAULT_SEED, first_index=0, stream=None):
        torch = _torch()
        dev = self.torch_device
        t32 = [torch.empty(max(count, 1), dtype=torch.int32, device=dev) for _ in range(2)]
        t16 = [torch.empty(max(count, 1), dtype=torch.int16, device=dev) for _ in range(3)]
        self._check(self.lib.nexg_gen_udp4_params(self.ctx, seed, first_index, count,
                                                  *[_ptr(t) for t in t32 + t16], self._stream(stream)))
        return [t[:count] for t in t32 + t16]


class FlowTable:
    """Per-flow counters across batches: a flow table kept in device memory
    (nexg_flow_entry rows, abi.FLOW_ENTRY_DTYPE, ascending by hash) in two
    buffers that swap at every update.

        table = FlowTable(eng, FlowOption(symmetric=True))
        for epoch, batch in enumerate(batches):
            rec = eng.parse(batch, out_kind=abi.OUT_RECORD)
            slot, group_of = table.update(batch, rec, epoch, min_epoch=max(epoch - 30, 0))
        rows = table.rows()
    """

    def __init__(self, engine: Engine, option=None, capacity: int = 1 << 16):
        self.engine = engine
        self.option = option
        self.capacity = max(int(capacity), 1)
        self.count = 0
        self._cur = self._buffer()
        self._next = self._buffer()

    def _buffer(self):
        return _torch().empty(self.capacity * 64, dtype=_torch().uint8, device=self.engine.torch_device)

    def update(self, batch: FrameBatch, records, epoch: int, min_epoch: int = 0, stream=None):
        """Count `batch` into the table: flow rows, sort, groups, merge
        (Engine.flow / flow_groups / flow_table_merge), then the buffers swap.
        `records` is the batch's NEXG_OUT_RECORD parse. Entries that no group
        of the batch matched and whose last_epoch is below min_epoch are
        dropped. When the new table does not fit, the capacity doubles until
        it does and the merge alone runs again (it is a pure function of its
        inputs). Returns (slot, group_of): int32 device tensors with the
        table position of every group's entry and the group of every frame,
        so frame i's entry is row slot[group_of[i]] of the new table."""
        eng = self.engine
        with eng._on(stream):  # the reallocation below follows `stream` too
            flows = eng.flow(batch, records, self.option, stream)
            groups, group_of, _, _ = eng.flow_groups(batch, records, flows, self.option, stream=stream)
            table = self._cur[: self.count * 64]
            while True:
                if self._next.numel() < self.capacity * 64:
                    self._next = self._buffer()
                _, n_out, slot = eng.flow_table_merge(batch, records, groups, table, epoch, min_epoch, self.option,
                                                      table_cap=self.capacity, out=self._next, stream=stream)
                if n_out <= self.capacity:
                    break
                while self.capacity < n_out:
                    self.capacity *= 2
        self._cur, self._next = self._next, self._cur
        self.count = n_out
        return slot, group_of

    def device_rows(self):
        """The table as a uint8 device tensor of `count` entries (a view of
        the current buffer: the update after next overwrites it)."""
        return self._cur[: self.count * 64]

    def rows(self):
        """The table on the host: an abi.FLOW_ENTRY_DTYPE array."""
        return self.device_rows().cpu().numpy().view(abi.FLOW_ENTRY_DTYPE).copy()
