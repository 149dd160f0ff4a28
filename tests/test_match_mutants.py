"""CPU: the strength of the match corpus (tests/match_frames.py), in the
manner of tests/test_second_pass_mutants.py. The GPU tests assert device ==
match_host on the corpus, so a one-token fault of the contract that the corpus
does not notice would not be noticed in the kernel either. For each entry of
MUTANTS match_host's source is taken, the old text replaced by the new one,
the variant built in a scratch namespace, and the corpus must hold a frame on
which the variant's row differs from the original's.

The corpus here is everything but the fuzz sets, and the first 150 frames of
each fuzz set (the variants run in plain Python): the sweep, the traps and the
shapes are what is meant to notice these faults. None of the seven is
equivalent: each changes the row of some frame of the corpus."""
import inspect

import pytest

from nex_amd import match as M
from tests import match_frames as mf

#: (name, old text, new text, which occurrence of the old text)
MUTANTS = [
    ("occurrence must end before the region's last byte", "q + L <= n", "q + L < n", 0),
    ("window: off_hi left out", "q <= p.off_hi", "q < p.off_hi", 0),
    ("fold reaches [", "0x5A", "0x5B", 0),
    ("fold reaches @", "0x41", "0x40", 0),
    ("tie goes to the highest index", "first_pat = min(", "first_pat = max(", 0),
    ("first_off relative to the region", "hits.append((start + q, i))", "hits.append((q, i))", 0),
    ("payload must end before the frame's last byte", "not off + ln <= length", "not off + ln < length", 0),
]


def variant(old, new, nth):
    src = inspect.getsource(M.match_host)
    parts = src.split(old)
    assert len(parts) > nth + 1, (old, "is not in the source")
    src = old.join(parts[: nth + 1]) + new + old.join(parts[nth + 1:])
    space = dict(M.__dict__)
    exec(compile(src, "<variant of match_host>", "exec"), space)
    return space["match_host"]


@pytest.fixture(scope="module")
def inputs(oracle):
    out = []
    for c in mf.cases():
        recs, rows = mf.expected(oracle, c)
        keep = range(len(c.frames)) if c.every_layout else range(150)
        out += [(c.frames[i], recs[i], len(c.frames[i]), c.pset, tuple(int(x) for x in rows[i].tolist()[:3])) for i in keep]
    return out


@pytest.mark.parametrize("name,old,new,nth", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_the_corpus_notices(inputs, name, old, new, nth):
    bad = variant(old, new, nth)
    for frame, rec, length, pset, want in inputs:
        try:
            got = bad(frame, rec, length, pset)
        except Exception:  # noqa: BLE001 - a variant that indexes past the frame is a detected fault
            return
        if got != want:
            return
    pytest.fail(f"no frame of the corpus notices: {name}")


def test_the_original_is_its_own_variant(inputs):
    same = variant("q + L <= n", "q + L <= n", 0)
    for frame, rec, length, pset, want in inputs[:500]:
        assert same(frame, rec, length, pset) == want
