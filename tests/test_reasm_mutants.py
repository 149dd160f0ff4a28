"""CPU: the strength of the reassembly corpus (tests/reasm_frames.py), in the
manner of tests/test_fragment_mutants.py. The GPU tests assert device ==
reassemble_host on the corpus, so a one-token fault of the contract that the
corpus does not notice would not be noticed in the kernels either. For each
entry of MUTANTS the source of nex_amd.reassemble is taken, the old text
replaced by the new one, the variant built in a scratch namespace, and the
corpus must hold a case at which the variant's outputs or rows differ from the
original's, at exact=False (what the device is held against) or exact=True.
EQUIVALENT lists the faults no input can show, each with the reason."""
import inspect

import pytest

from nex_amd import reassemble as R
from tests import reasm_frames as rf

#: (name, old text, new text, which occurrence of the old text)
MUTANTS = [
    ("d >= 8 becomes d > 8", "or d0 < 8:", "or d0 <= 8:", 0),
    ("no lower bound on a piece in front of another", "or d0 < 8:", "or d0 < 0:", 0),
    ("contiguity not tested", "if 8 * fo1 != 8 * fo0 + d0 or", "if", 0),
    ("an overlap is let through", "8 * fo1 != 8 * fo0 + d0", "8 * fo1 > 8 * fo0 + d0", 0),
    ("a gap is let through", "8 * fo1 != 8 * fo0 + d0", "8 * fo1 < 8 * fo0 + d0", 0),
    ("MF in the middle not tested", "        if not mf0:\n            return False\n", "", 0),
    ("MF on the last not tested", "if mf_last or d_last < 1:", "if d_last < 1:", 0),
    ("an empty last piece is let through", "if mf_last or d_last < 1:", "if mf_last:", 0),
    ("member 0 need not start at 0", "if members[0][1] != 0:", "if False:", 0),
    ("<= 65535 becomes < 65535", "8 * fo_last + d_last <= 65535", "8 * fo_last + d_last < 65535", 0),
    ("the last member's header length in the size rule", "return members[0][0] + 8 * fo_last", "return hl_last + 8 * fo_last", 0),
    ("the flags mask 0xC000 becomes 0xE000", "& 0xC000)", "& 0xE000)", 0),
    ("the flags mask 0xC000 becomes 0x4000", "& 0xC000)", "& 0x4000)", 0),
    ("the flags mask 0xC000 becomes 0x8000", "& 0xC000)", "& 0x8000)", 0),
    ("whole: the MF bit alone", "if word & 0x3FFF == 0:", "if word & 0x2000 == 0:", 0),
    ("whole: the offset alone", "if word & 0x3FFF == 0:", "if word & 0x1FFF == 0:", 0),
    ("the identification is not in the key", "f[23], _be16(f, 18))", "f[23], 0)", 0),
    ("the source is not in the key", "key = (f[26:30],", "key = (b'',", 0),
    ("the destination is not in the key", "f[30:34], f[23]", "b'', f[23]", 0),
    ("the members ordered by frame number alone", "key=lambda i: (cls[i][3], i)", "key=lambda i: i", 0),
    ("a part's own header length places its data", "14 + hl:14 + hl + d]", "14 + hl0:14 + hl0 + d]", 0),
    ("bytes past the total length are data", "return abi.FRAME_OK, abi.REASM_HELD, hl, word & 0x1FFF, (word >> 13) & 1, total - hl, key",
     "return abi.FRAME_OK, abi.REASM_HELD, hl, word & 0x1FFF, (word >> 13) & 1, n - 14 - hl, key", 0),
    ("the checksum is kept", "    h[10:12] = header_checksum(bytes(h)).to_bytes(2, \"big\")\n", "", 0),
    ("the total length is the head's", "    h[2:4] = (hl0 + size).to_bytes(2, \"big\")\n", "", 0),
    ("a collision is not flagged", "rows[\"flags\"][idx] = abi.REASM_COLLISION", "pass", 0),
    ("a mixed run is reassembled on the device", "            if not exact:\n", "            if False:\n", 0),
    ("the protocol is not in the key", "f[30:34], f[23], _be16", "f[30:34], 0, _be16", 0),
    ("TL == hl is no IPv4", "if total < hl or", "if total <= hl or", 0),
]

#: faults that no table can show, and why
EQUIVALENT = [
    ("the identification is hashed", "+ bytes([0, key[2], 0, 0]))", "+ bytes([0, key[2]]) + key[3].to_bytes(2, 'big'))",
     "a run is keyed by (hash, identification): two keys of one identification whose hashes are equal without it are "
     "equal with it, the hash being linear, so no run changes"),
    ("a frame of 33 bytes is looked into", "if n < 34 or", "if n < 33 or",
     "IHL >= 5 makes 14 + hl >= 34, so the next test passes every frame under 34 bytes through as well"),
]


def variant(old, new, nth):
    src = inspect.getsource(R)
    parts = src.split(old)
    assert len(parts) > nth + 1, (old, "is not in the source")
    src = old.join(parts[: nth + 1]) + new + old.join(parts[nth + 1:])
    space = {"__name__": "variant_of_nex_amd_reassemble", "__package__": "nex_amd"}
    exec(compile(src, "<variant of nex_amd.reassemble>", "exec"), space)
    return space["reassemble_host"]


@pytest.fixture(scope="module")
def inputs():
    """Every case under 4200 bytes a frame and the two 65535 / 65536 cases (the variants run in plain Python), with
    the original's output both ways."""
    tables = [fs for name, _, fs in rf.cases() if all(f is None or len(f) < 4200 for f in fs) or "6553" in name]
    return [(fs, exact, R.reassemble_host(fs, 1, exact)) for fs in tables for exact in (False, True)]


def differs(a, b):
    return a[0] != b[0] or a[1].tolist() != b[1].tolist() or a[2].tobytes() != b[2].tobytes() or a[3].tolist() != b[3].tolist()


@pytest.mark.parametrize("name,old,new,nth", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_the_corpus_notices(inputs, name, old, new, nth):
    bad = variant(old, new, nth)
    for frames, exact, want in inputs:
        try:
            got = bad(frames, 1, exact)
        except Exception:  # a variant that raises shows nothing
            continue
        if differs(got, want):
            return
    pytest.fail(f"no case of the corpus notices: {name}")


@pytest.mark.parametrize("name,old,new,why", EQUIVALENT, ids=[m[0] for m in EQUIVALENT])
def test_the_listed_faults_are_not_noticed(inputs, name, old, new, why):
    """A listed fault that the corpus came to notice belongs in MUTANTS."""
    bad = variant(old, new, 0)
    assert why and not any(differs(bad(frames, 1, exact), want) for frames, exact, want in inputs)


def test_the_original_is_its_own_variant(inputs):
    same = variant("or d0 < 8:", "or d0 < 8:", 0)
    for frames, exact, want in inputs:
        assert not differs(same(frames, 1, exact), want)
