"""GPU: reassembly of trains whose pieces lie on both sides of a 4-GiB offset
(tests/far_batch.py's buffer size and boundaries): the classification, the
header staging and the data copies all make source addresses below and above
2^32 inside one datagram, and one piece straddles the boundary itself. Output
frames, table and rows must equal reassemble_host over the same frames."""
import numpy as np
import pytest

from nex_amd import abi
from nex_amd.engine import FrameBatch
from nex_amd.reassemble import Reassembler, pack_host, reassemble_host
from tests import far_batch as fb
from tests import fragment_frames as ff
from tests import helpers
from tests import reasm_frames as rf

pytestmark = pytest.mark.gpu


def test_a_train_on_both_sides_of_4_gib(engine):
    import torch
    try:
        buf = torch.empty(fb.BUFFER_BYTES, dtype=torch.uint8, device="cuda")
    except (RuntimeError, torch.cuda.OutOfMemoryError) as e:
        pytest.skip(f"a {fb.BUFFER_BYTES}-B device allocation was refused: {e}")
    a = rf.train(ff.ipv4(3000, ff.RA, seed=31), 576, 0x6101)   # six pieces
    b = rf.train(ff.ipv4(1700, seed=32), 576, 0x6102)          # four, the last one missing
    frames = [a[3], b[1], a[0], ff.ipv4(90, seed=33), a[5], b[0], a[1], a[4], b[2], a[2]]
    # odd pieces below the boundary, even ones above, frame 6 across it, at every byte phase
    offs = np.zeros(len(frames), np.int64)
    low, high = fb.GIB4 - 70000, fb.GIB4 + 4097
    for i, f in enumerate(frames):
        if i == 6:
            offs[i] = fb.GIB4 - 301
        elif i % 2:
            offs[i], low = low, low + len(f) + 1 + i
        else:
            offs[i], high = high, high + len(f) + 3 + i
    assert offs[6] < fb.GIB4 < offs[6] + len(frames[6]) and offs.max() + 2000 < fb.BUFFER_BYTES
    for o, f in zip(offs, frames):
        buf[int(o):int(o) + len(f)] = torch.from_numpy(np.frombuffer(f, np.uint8).copy()).cuda()
    batch = FrameBatch(data=buf, count=len(frames), offsets=torch.from_numpy(offs).cuda(),
                       lengths=torch.from_numpy(np.array([len(f) for f in frames], np.int32)).cuda())
    out_frames, src, rows, _ = reassemble_host(frames, exact=False)
    assert list(rows["kind"]) == [abi.REASM_PART, abi.REASM_HELD, abi.REASM_HEAD, abi.REASM_PASS, abi.REASM_PART, abi.REASM_HELD,
                                  abi.REASM_PART, abi.REASM_PART, abi.REASM_HELD, abi.REASM_PART]
    for align in (1, 16):
        out, d_src, d_rows, (hidx, held) = Reassembler(engine).run(batch, align)
        torch.cuda.synchronize()
        data, o = pack_host(out_frames, align)
        assert (helpers.to_host(d_rows, abi.REASM_DTYPE, len(frames)) == rows).all(), align
        assert (out.offsets.cpu().numpy() == o).all() and out.data.cpu().numpy().tobytes() == data, align
        assert (d_src.cpu().numpy().view(np.uint32) == src).all() and list(hidx.cpu().numpy()) == [1, 5, 8], align
        assert (held.offsets.cpu().numpy() == offs[[1, 5, 8]]).all(), align
    del buf, batch
    torch.cuda.empty_cache()
