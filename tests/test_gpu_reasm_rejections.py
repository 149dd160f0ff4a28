"""GPU: what nexg_reasm_plan / nexg_reasm_frames / nexg_reasm_held reject, what
they do with an empty table, and what nexg_reasm_frames does with rows,
out_first and out_bytes that lie. The lying inputs stay inside tensors the test
owns and the outputs stand between guard bands that are checked on the host
after a synchronise: no out-of-range pointer is passed."""
import ctypes

import numpy as np
import pytest

from nex_amd import abi
from nex_amd.engine import FrameBatch
from nex_amd.reassemble import pack_host, reassemble_host
from tests import fragment_frames as ff
from tests import reasm_frames as rf

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 4096


def P(t, skew=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + skew)


def table():
    """Seven datagrams of three or four pieces and some whole frames, shuffled: 64 frames."""
    import random
    frames = []
    for k in range(7):
        frames += rf.train(ff.ipv4(1200 + 160 * k, ff.RA if k % 2 else b"", seed=k), 576, 0x5000 + k)
    frames += [ff.ipv4(40 + 9 * k, seed=k) for k in range(64 - len(frames))]
    random.Random(2).shuffle(frames)
    return frames


def buffers(n, k, total):
    import torch
    t = lambda count, dtype, fill: torch.full((count,), fill, dtype=dtype, device="cuda")  # noqa: E731
    return dict(first=t(n + 3, torch.int32, -1), nbytes=t(n + 3, torch.int64, -1), rows=t((n + 2) * 16, torch.uint8, FILL),
                off=t(k + 3, torch.int64, -1), len=t(k + 2, torch.int32, -1), src=t(k + 2, torch.int32, -1),
                out=t(total + 2 * GUARD, torch.uint8, FILL))


def plan_args(engine, batch, b, ws, ws_bytes, align=1):
    return [engine.ctx, ctypes.byref(batch.to_c()), align, P(b["first"]), P(b["nbytes"]), P(b["rows"]), P(ws), ws_bytes,
            engine._stream(None)]


def frames_args(engine, batch, b, k, total, align=1):
    return [engine.ctx, ctypes.byref(batch.to_c()), align, P(b["rows"]), P(b["first"]), P(b["nbytes"]), k, P(b["off"]),
            P(b["len"]), P(b["src"]), P(b["out"], GUARD), total, engine._stream(None)]


def test_rejected_arguments(engine):
    import torch
    frames = table()
    n = len(frames)
    batch = FrameBatch.from_frames(frames)
    out_frames, src, rows, _ = reassemble_host(frames, exact=False)
    k, total = len(out_frames), sum(len(f) for f in out_frames)
    b = buffers(n, k, total)
    ws_bytes = abi.reasm_plan_workspace(n)
    ws = torch.empty(ws_bytes + 16, dtype=torch.uint8, device="cuda")
    lib = engine.lib
    good = plan_args(engine, batch, b, ws, ws_bytes)
    assert lib.nexg_reasm_plan(*good) == abi.OK
    for at, bad in ((0, None), (1, None), (2, 0), (2, 2), (2, 32), (3, None), (4, None), (5, None), (6, None), (7, ws_bytes - 1),
                    (3, P(b["first"], 2)), (4, P(b["nbytes"], 4)), (5, P(b["rows"], 8)), (6, P(ws, 8))):
        args = list(good)
        args[at] = bad
        assert lib.nexg_reasm_plan(*args) == abi.EINVAL, ("plan", at, bad)
    good = frames_args(engine, batch, b, k, total)
    assert lib.nexg_reasm_frames(*good) == abi.OK
    for at, bad in ((0, None), (1, None), (2, 3), (3, None), (4, None), (5, None), (6, 1 << 32), (7, None), (8, None), (9, None),
                    (10, None), (3, P(b["rows"], 8)), (4, P(b["first"], 2)), (5, P(b["nbytes"], 4)), (7, P(b["off"], 4)),
                    (8, P(b["len"], 2)), (9, P(b["src"], 2)), (10, P(b["out"], GUARD + 8))):
        args = list(good)
        args[at] = bad
        assert lib.nexg_reasm_frames(*args) == abi.EINVAL, ("frames", at, bad)
    hw_bytes = abi.reasm_held_workspace(n)
    hw = torch.empty(hw_bytes + 16, dtype=torch.uint8, device="cuda")
    idx, off, ln = engine._table(n)
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    good = [engine.ctx, ctypes.byref(batch.to_c()), P(b["rows"]), n, P(idx), P(off), P(ln), P(cnt), P(hw), hw_bytes,
            engine._stream(None)]
    assert lib.nexg_reasm_held(*good) == abi.OK
    for at, bad in ((0, None), (1, None), (2, None), (3, n - 1), (4, None), (5, None), (6, None), (7, None), (8, None),
                    (9, hw_bytes - 1), (2, P(b["rows"], 8)), (4, P(idx, 2)), (5, P(off, 4)), (6, P(ln, 2)), (7, P(cnt, 4)),
                    (8, P(hw, 2))):
        args = list(good)
        args[at] = bad
        assert lib.nexg_reasm_held(*args) == abi.EINVAL, ("held", at, bad)
    torch.cuda.synchronize()
    assert int(cnt[0]) == int((rows["kind"] == abi.REASM_HELD).sum())


def test_an_empty_table(engine):
    import torch
    empty = FrameBatch.from_frames([])
    b = buffers(0, 0, 0)
    lib = engine.lib
    args = plan_args(engine, empty, b, None, 0)
    args[5] = None  # no rows, no workspace
    assert lib.nexg_reasm_plan(*args) == abi.OK
    args = frames_args(engine, empty, b, 0, 0)
    args[3] = args[8] = args[9] = args[10] = None
    assert lib.nexg_reasm_frames(*args) == abi.OK
    cnt = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    hw = torch.empty(abi.reasm_held_workspace(0), dtype=torch.uint8, device="cuda")
    assert lib.nexg_reasm_held(engine.ctx, ctypes.byref(empty.to_c()), None, 0, None, None, None, P(cnt), P(hw), hw.numel(),
                               engine._stream(None)) == abi.OK
    torch.cuda.synchronize()
    assert b["first"].cpu().numpy()[0] == 0 and (b["first"].cpu().numpy()[1:] == -1).all()
    assert b["nbytes"].cpu().numpy()[0] == 0 and (b["nbytes"].cpu().numpy()[1:] == -1).all()
    assert b["off"].cpu().numpy()[0] == 0 and (b["off"].cpu().numpy()[1:] == -1).all()
    assert (b["out"].cpu().numpy() == FILL).all() and list(cnt.cpu().numpy()) == [0, -1]
    from nex_amd.reassemble import Reassembler
    out, src, rows, (hidx, held) = Reassembler(engine).run(empty)
    assert out.count == 0 and src.numel() == 0 and rows.numel() == 0 and held.count == 0


def test_lying_rows_first_and_bytes_store_nothing_outside_the_documented_ranges(engine):
    import torch
    frames = table()
    n = len(frames)
    batch = FrameBatch.from_frames(frames)
    out_frames, src, rows, _ = reassemble_host(frames, exact=False)
    data, offs = pack_host(out_frames, 1)
    honest = np.frombuffer(data, np.uint8)
    k, total = len(out_frames), len(honest)
    first_of = np.concatenate([np.where(np.isin(rows["kind"], (abi.REASM_PASS, abi.REASM_HEAD)), rows["out"], 0), [k]]).astype(np.int64)
    for i in range(n - 1, -1, -1):  # out_first: the output frames before i
        if rows["kind"][i] not in (abi.REASM_PASS, abi.REASM_HEAD):
            first_of[i] = first_of[i + 1]
    byte_of = offs[first_of]
    heads = np.flatnonzero(rows["kind"] == abi.REASM_HEAD)
    parts = lambda h: [i for i in np.flatnonzero(rows["head"] == h) if i != h]  # noqa: E731
    h0, h1, h2, h3, h4, h5, h6 = heads[:7]
    lie_rows, lie_first, lie_bytes = rows.copy(), first_of.copy(), byte_of.copy()
    moved = parts(h0)[0]
    lie_rows["head"][moved] = h1                       # a part names another datagram's head
    lie_rows["head"][parts(h2)[0]] = 0xFFFFFFF0        # a head past the table
    lie_rows["kind"][parts(h3)[-1]] = abi.REASM_HEAD   # a part that says it is a head
    lie_rows["data_len"][h4] = 0xFFFF                  # a head with a D that is not its datagram's
    lie_bytes[h5 + 1] = byte_of[h5] + 300              # the head's room ends inside its own data
    lie_bytes[h6] = total + 100000                     # a datagram that starts past the capacity
    whole = int(np.flatnonzero(rows["kind"] == abi.REASM_PASS)[5])
    lie_first[whole + 1] = lie_first[whole]            # a pass-through that may write no table entry
    b = buffers(n, k, total)
    b["rows"][: n * 16] = torch.from_numpy(lie_rows.view(np.uint8).copy()).cuda()
    b["first"][: n + 1] = torch.from_numpy(lie_first.astype(np.int32)).cuda()
    b["nbytes"][: n + 1] = torch.from_numpy(lie_bytes).cuda()
    cut = k - 1                                        # out_count one below the table
    assert engine.lib.nexg_reasm_frames(*frames_args(engine, batch, b, cut, total)) == abi.OK
    torch.cuda.synchronize()
    got = b["out"].cpu().numpy()
    assert (got[:GUARD] == FILL).all() and (got[GUARD + total:] == FILL).all(), "a store outside out_data or at or past out_cap"
    got = got[GUARD:GUARD + total]
    # the ranges a lie may have changed: the named heads', and those whose neighbours' out_bytes moved
    touched = {int(rows["out"][h]) for h in (h0, h1, h2, h3, h4, h5, h6)}
    for f in (int(rows["out"][h5]), int(rows["out"][h6])):
        touched |= {f - 1, f + 1}                      # frames h5 + 1 and h6 - 1 take their room from the moved entries
    touched |= {int(first_of[h5 + 1]), int(first_of[h6]) - 1}
    for f in range(k):
        if f not in touched:
            assert got[offs[f]:offs[f + 1]].tobytes() == honest[offs[f]:offs[f + 1]].tobytes(), f
    # h0's range: everything but the moved part's bytes is honest, those are untouched
    o0 = int(offs[rows["out"][h0]])
    fo, d = int.from_bytes(frames[moved][20:22], "big") & 0x1FFF, int.from_bytes(frames[moved][16:18], "big") - 4 * (frames[moved][14] & 15)
    at = o0 + 14 + int(rows["hdr_len"][h0]) + 8 * fo
    assert (got[at:at + d] == FILL).all() and got[o0:at].tobytes() == honest[o0:at].tobytes()
    # h2 and h3 miss one part each, h4's header carries the lie and nothing else does
    for h in (h2, h3):
        o = int(offs[rows["out"][h]])
        assert got[o:o + 14 + int(rows["hdr_len"][h])].tobytes() == honest[o:o + 14 + int(rows["hdr_len"][h])].tobytes()
    o4, e4 = int(offs[rows["out"][h4]]), int(offs[rows["out"][h4] + 1])
    same = np.ones(e4 - o4, bool)
    same[[16, 17, 24, 25]] = False
    assert (got[o4:e4][same] == honest[o4:e4][same]).all()
    # h5 stops at its moved end, h6 writes nothing
    o5 = int(offs[rows["out"][h5]])
    assert got[o5:o5 + 300].tobytes() == honest[o5:o5 + 300].tobytes()
    o6, e6 = int(offs[rows["out"][h6]]), int(offs[rows["out"][h6] + 1])
    assert (got[o6 + 15:e6] == FILL).all()            # the frame in front, given its room, may zero up to 15 pad bytes
    # the tables: nothing at or past out_count, nothing for the pass-through without room
    h_off, h_len, h_src = b["off"].cpu().numpy(), b["len"].cpu().numpy(), b["src"].cpu().numpy()
    assert (h_len[cut:] == -1).all() and (h_src[cut:] == -1).all() and (h_off[cut + 1:] == -1).all()
    assert h_off[cut] == lie_bytes[n]
    f = int(rows["out"][whole])
    assert h_src[f] != whole
    ok = [f for f in range(cut) if src[f] not in (whole, whole + 1, h4) and f not in touched]
    assert (h_src[ok].view(np.uint32) == src[ok]).all() and (h_len[ok] == np.array([len(out_frames[f]) for f in ok])).all()
