"""CPU: the strength of the fragmentation corpus (tests/fragment_frames.py), in
the manner of tests/test_match_mutants.py. The GPU tests assert device ==
fragment_host on the corpus, so a one-token fault of the contract that the
corpus does not notice would not be noticed in the kernel either. For each
entry of MUTANTS the source of nex_amd.fragment is taken, the old text replaced
by the new one, the variant built in a scratch namespace, and the corpus must
hold a frame and an mtu at which the variant's pieces or rows differ from the
original's. None of the seven is equivalent."""
import inspect

import pytest

from nex_amd import fragment as F
from tests import fragment_frames as ff

#: (name, old text, new text, which occurrence of the old text)
MUTANTS = [
    ("piece data not rounded down to 8", "p = (mtu - hl) & ~7", "p = (mtu - hl)", 0),
    ("a frame of exactly the mtu is split", "if total <= mtu:", "if total < mtu:", 0),
    ("the input's own offset is not added", "more | (fo0 + k * p // 8)", "more | (k * p // 8)", 0),
    ("the last piece's MF forced to 0", "if k < count - 1 else mf0", "if k < count - 1 else 0", 0),
    ("the copied bit read the wrong way round", "if not t & 0x80:", "if t & 0x80:", 0),
    ("piece 0's options NOP-filled too", "        if k:\n", "        if True:\n", 0),
    ("DF ignored", "if df and not ignore_df:", "if False:", 0),
]
MTUS = (68, 576, 1500)


def variant(old, new, nth):
    src = inspect.getsource(F)
    parts = src.split(old)
    assert len(parts) > nth + 1, (old, "is not in the source")
    src = old.join(parts[: nth + 1]) + new + old.join(parts[nth + 1:])
    space = {"__name__": "variant_of_nex_amd_fragment", "__package__": "nex_amd"}
    exec(compile(src, "<variant of nex_amd.fragment>", "exec"), space)
    return space["fragment_host"]


@pytest.fixture(scope="module")
def inputs():
    """The corpus without its two 65535-byte frames (the variants run in plain Python), and the original's output."""
    frames = [f for f in ff.frames() if f is None or len(f) < 30000]
    return frames, {(m, i): F.fragment_host(frames, m, i) for m in MTUS for i in (False, True)}


def differs(a, b):
    return a[0] != b[0] or a[1].tolist() != b[1].tolist() or a[2].tobytes() != b[2].tobytes()


@pytest.mark.parametrize("name,old,new,nth", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_the_corpus_notices(inputs, name, old, new, nth):
    bad = variant(old, new, nth)
    frames, want = inputs
    for (mtu, ignore), w in want.items():
        if differs(bad(frames, mtu, ignore), w):  # an output that differs: a variant that raised would not count
            return
    pytest.fail(f"no frame of the corpus notices: {name}")


def test_the_original_is_its_own_variant(inputs):
    same = variant("if total <= mtu:", "if total <= mtu:", 0)
    frames, want = inputs
    for (mtu, ignore), w in want.items():
        assert not differs(same(frames, mtu, ignore), w)
