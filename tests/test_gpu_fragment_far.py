"""GPU: fragmentation of batches whose frame offsets cross 2^31 and 2^32
(tests/far_batch.py's placements, placed as tests/test_gpu_far_batch.py places
them: one corpus at byte 1, around 2^31 and around 2^32 of a buffer of 2^32 +
2 MiB bytes). Table forms 1 (u64 offsets + lengths) and 2 (its u32 table with
group bases), mtu 576: the shape reads, the header staging and the piece copy
all make source addresses at and above 2^31 and 2^32, with a frame that
straddles each boundary (placement C: the 65535-byte one, 119 pieces). Output
frames, table and rows must equal fragment_host over the same frames."""
import numpy as np
import pytest

from nex_amd import abi
from nex_amd.fragment import fragment_frame, plan_host
from tests import far_batch as fb
from tests import helpers
from tests import test_gpu_far_batch as far_gpu

pytestmark = pytest.mark.gpu

MTU = 576
dev = far_gpu.dev  # the module-scoped buffer fixture, a fresh one for this module


@pytest.fixture(scope="module")
def per_id():
    """fragment_frame of every distinct frame of the far batch."""
    return [fragment_frame(f, MTU, True) for f in fb.far().frames]  # most of the corpus has DF set


def expected(per_id, ids, align):
    pieces, src = [], []
    rows = np.zeros(len(ids), abi.FRAGGED_DTYPE)
    for i, c in enumerate(ids):
        p, status, kind, hl, pd = per_id[int(c)]
        rows[i] = (status, kind, hl, 0, len(p), pd, len(pieces), 0)
        pieces += p
        src += [i] * len(p)
    return pieces, np.array(src, np.uint32), rows, plan_host([len(p) for p in pieces], align)


@pytest.mark.parametrize("name", fb.PLACEMENTS)
def test_fragment(engine, dev, per_id, name):
    import torch
    pl = dev.far.placements[name]
    tables = dev.tables(name, forms=(1, 2), hints=False, views=False)
    assert [t.name.split()[1] for t in tables] == ["1", "2"]
    for t, align in zip(tables, (1, 16)):
        pieces, src, rows, offs = expected(per_id, t.ids, align)
        assert int((rows["kind"] == abi.FRAG_SPLIT).sum()) >= 6, "the far corpus has frames over the mtu in every cluster"
        for b in fb.BOUNDARIES:  # a split frame lies on or above each boundary, and one reaches across it in C
            r = pl.row[b]
            assert t.off[r] + pl.length[r] > b
            assert ((t.off >= b) & (rows["kind"] == abi.FRAG_SPLIT)).any(), (name, b)
            if name == "C":
                assert t.off[r] < b and rows["kind"][r] == abi.FRAG_SPLIT and rows["pieces"][r] > 100
        out, d_src, d_rows = engine.fragment(t.batch, MTU, ignore_df=True, align=align)
        torch.cuda.synchronize()
        what = f"{name} {t.name} align {align}"
        far_gpu.rows_equal(helpers.to_host(d_rows, abi.FRAGGED_DTYPE, len(rows)), rows, what)
        assert out.count == len(pieces) and (out.offsets.cpu().numpy() == offs).all(), what
        assert (d_src.cpu().numpy().view(np.uint32) == src).all(), what
        if align != 1:
            assert (out.lengths.cpu().numpy() == [len(p) for p in pieces]).all(), what
        want = np.zeros(int(offs[-1]), np.uint8)
        for o, p in zip(offs[:-1], pieces):
            want[o:o + len(p)] = np.frombuffer(p, np.uint8)
        got = out.data.cpu().numpy()
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (what, len(bad), int(bad[0]), int(np.searchsorted(offs, bad[0], side="right")) - 1)
