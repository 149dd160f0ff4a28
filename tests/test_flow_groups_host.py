"""CPU: the host contract of the per-flow counters (nex_amd.flow.sort_host /
groups_host restate nexg_flow_sort / nexg_flow_groups of include/nexg.h).

- against the independent reference of tests/flow_group_frames.py (a dict
  group-by over the hash with a set of keys per group, on
  tests/second_pass_ref.py's hash and address code) on the hand corpus and the
  fuzz corpus's flow frames, under the four symmetric x ports options; some
  frames of each corpus are given a bad extent (no bytes, or a length over
  65535) so that `bytes` has something to leave out;
- the pinned 32-bit collision: two address pairs, one hash, one group, mixed;
- order entries past the batch and a caller's own order;
- the ABI: struct size, offsets and both workspace helpers of abi.py equal the
  header's (tests/native/cpp_flow_groups_test --link);
- seeded faults in groups_host that the corpus must notice, in the way of
  tests/test_second_pass_mutants.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from nex_amd import abi
from nex_amd import flow as hostflow
from nex_amd.flow import FlowOption, groups_host, sort_host
from tests import flow_frames as ff
from tests import flow_group_frames as fg
from tests import helpers
from tests import second_pass_fuzz as fz
from tests import second_pass_ref as ref
from tests.test_second_pass_mutants import variant

OPTIONS = [(s, p) for s in (False, True) for p in (True, False)]
WORKSPACE_COUNTS = [0, 1, 255, 256, 257, 511, 512, 513, 1024, 65793, 262145, 1048577, (1 << 32) - 1]


def with_bad_extents(frames):
    """(frames, lengths): every 11th frame loses its bytes (an extent outside
    the data; the table still gives its length), every 13th gets a table
    length over 65535."""
    frames, lengths = list(frames), [len(f) for f in frames]
    for i in range(3, len(frames), 11):
        frames[i] = None
    for i in range(5, len(frames), 13):
        lengths[i] += 65536
    return frames, lengths


class Inputs:
    def __init__(self, oracle, frames, flags):
        self.recs = oracle.parse_frames(frames, flags)
        self.frames, self.lengths = with_bad_extents(frames)
        self.count = len(frames)
        self.flows = {(s, p): ref.flow_rows(self.frames, self.recs, self.lengths, s, p) for s, p in OPTIONS}

    def args(self, s, p):
        return self.frames, self.recs, self.lengths, self.flows[(s, p)], FlowOption(symmetric=s, ports=p)


@pytest.fixture(scope="module")
def hand(oracle):
    return Inputs(oracle, [x.frame for x in ff.corpus()] + fg.collision_frames(), ff.PARSE_FLAGS)


@pytest.fixture(scope="module")
def fuzz(oracle):
    return Inputs(oracle, fz.corpora(oracle).flow + fg.collision_frames(), fz.SELECT_PARSE_FLAGS)


def test_sort_host_orders_by_hash_then_frame():
    rng = np.random.default_rng(3)
    h = rng.integers(0, 1 << 32, 5000, dtype=np.uint64).astype(np.uint32)
    h[::7] = 0xFFFFFFFF
    h[3::5] = 0
    h[1::9] = h[0]
    order = sort_host(h)
    assert order.dtype == np.uint32
    assert order.tolist() == sorted(range(len(h)), key=lambda i: (int(h[i]), i))
    assert sort_host(np.zeros(0, np.uint32)).tolist() == []
    assert sort_host(np.full(100, 7, np.uint32)).tolist() == list(range(100))


@pytest.mark.parametrize("which", ["hand", "fuzz"])
@pytest.mark.parametrize("symmetric,ports", OPTIONS)
def test_groups_host_against_the_reference(request, which, symmetric, ports):
    inp = request.getfixturevalue(which)
    args = inp.args(symmetric, ports)
    want = fg.ref_groups(inp.frames, inp.recs, inp.lengths, args[3], symmetric, ports)
    groups, group_of, n = groups_host(*args)
    order = sort_host(args[3]["hash"])
    fg.check_against_ref(groups, group_of, n, order, want, inp.count)
    # the corpus has what the counters are about
    assert (groups["packets"] > 1).sum() > 5 and (groups["mixed"] > 0).sum() >= 1
    skipped = sum(int(ln) for f, ln in zip(inp.frames, inp.lengths) if f is None or ln > 65535)
    assert skipped > 0 and int(groups["bytes"].sum()) == sum(int(x) for x in inp.lengths) - skipped


def test_the_collision_pair_is_one_mixed_group(oracle):
    """10.0.0.1 -> 10.0.0.2 and 231.24.44.220 -> 10.0.0.2 hash alike under the
    default key, with and without the (equal) ports."""
    a, b = (b"".join(ff.ip(x) for x in pair) for pair in (fg.COLLISION_A, fg.COLLISION_B))
    assert hostflow.toeplitz(a) == hostflow.toeplitz(b) == fg.COLLISION_HASH
    assert ref.toeplitz_shift(a, hostflow.DEFAULT_KEY) == fg.COLLISION_HASH
    ports = b"".join(p.to_bytes(2, "big") for p in fg.COLLISION_PORTS)
    assert hostflow.toeplitz(a + ports) == hostflow.toeplitz(b + ports)
    for pattern, mixed in (("AB", 1), ("ABAAB", 3), ("AAAAA", 0), ("BBAAA", 1)):
        frames = fg.collision_frames(pattern)
        recs = oracle.parse_frames(frames, ff.PARSE_FLAGS)
        lengths = [len(f) for f in frames]
        flows = hostflow.flows_host(frames, recs, lengths)
        assert len(set(flows["hash"].tolist())) == 1 and int(flows["kind"][0]) == abi.FLOW_IPV4_L4
        groups, group_of, n = groups_host(frames, recs, lengths, flows)
        assert n == 1 and group_of.tolist() == [0] * len(frames)
        g = groups[0]
        assert (int(g["packets"]), int(g["mixed"]), int(g["flags8"])) == (len(frames), mixed, 1 if mixed else 0), pattern
        assert int(g["hash"]) == hostflow.toeplitz(a + ports) and int(g["bytes"]) == sum(lengths)
        assert (int(g["first"]), int(g["first_index"]), int(g["kind"]), int(g["proto"])) == (0, 0, abi.FLOW_IPV4_L4, 17)


def test_a_callers_order(hand):
    """Entries past the batch are frames with an all-zero row, no key and no
    length; they join the run of hash 0 they stand in and get no group_of
    entry. Any order is taken as it is: groups are runs."""
    args = hand.args(False, True)
    n = hand.count
    order = sort_host(args[3]["hash"])
    none = int((args[3]["hash"] == 0).sum())
    assert none >= 2
    hostile = np.concatenate([np.array([n, 0xFFFFFFFF], np.uint32), order[: n - 2]])
    groups, group_of, count = groups_host(*args, order=hostile)
    plain, plain_of, plain_count = groups_host(*args)
    assert 0 < count <= plain_count and int(groups[0]["hash"]) == 0 and plain_of.max() == plain_count - 1
    assert int(groups[0]["packets"]) == none + 2 and int(groups[0]["first_index"]) == n
    assert (int(groups[0]["kind"]), int(groups[0]["proto"])) == (0, 0)
    left_out = order[n - 2:]
    assert (group_of[left_out] == 0xFFFFFFFF).all()
    # the identity order: runs of equal hashes between neighbours in frame order
    groups, group_of, count = groups_host(*args, order=np.arange(n, dtype=np.uint32))
    h = args[3]["hash"]
    assert count == 1 + int((h[1:] != h[:-1]).sum()) and int(groups["packets"].sum()) == n
    assert (groups["first_index"] == groups["first"]).all()


def test_abi_matches_the_header():
    exe = helpers.build_native_test("cpp_flow_groups_test")
    r = subprocess.run([exe, "--link"] + [str(c) for c in WORKSPACE_COUNTS], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0].split() == ["link", "ok", "3"]
    tok = lines[1].split()
    got = dict(zip(tok[0::2], (int(x) for x in tok[1::2])))
    assert got.pop("struct") == abi.FLOW_GROUP_DTYPE.itemsize == 32
    assert got == {n: abi.FLOW_GROUP_DTYPE.fields[n][1] for n in abi.FLOW_GROUP_DTYPE.names}
    assert [l.split() for l in lines[2:]] == [["workspace", str(c), str(abi.flow_sort_workspace(c)),
                                               str(abi.flow_groups_workspace(c))] for c in WORKSPACE_COUNTS]
    for c in WORKSPACE_COUNTS:
        assert abi.flow_sort_workspace(c) % 8 == 0 and abi.flow_groups_workspace(c) % 8 == 0


def test_header_declares_and_library_exports():
    root = ff.ROOT
    text = open(os.path.join(root, "include", "nexg.h")).read()
    for fn in ("nexg_flow_sort", "nexg_flow_groups"):
        assert re.search(r"^int " + fn + r"\(nexg_ctx\* ctx,", text, re.M), fn
        assert fn in abi.EXPORTED_SYMBOLS
    assert {"nexg_flow_sort_workspace", "nexg_flow_groups_workspace"} <= set(abi.HEADER_INLINE)
    assert re.search(r"#define NEXG_ABI_VERSION 1\b", text)
    from nex_amd import _lib
    lib = _lib.load()
    for fn in ("nexg_flow_sort", "nexg_flow_groups"):
        assert getattr(lib, fn).restype is ctypes.c_int
    # without a context the entries refuse cleanly
    assert lib.nexg_flow_sort(None, None, 0, None, None, 0, None) == abi.EINVAL
    assert lib.nexg_flow_groups(None, None, None, None, None, None, None, 0, None, None, None, 0, None) == abi.EINVAL


# ---- seeded faults ---------------------------------------------------------------------------------

#: (name, old text, new text) in groups_host's source
MUTANTS = [
    ("keys compared without proto", "elif key != prev[1]:", "elif (key[0], key[2]) != (prev[1][0], prev[1][2]):"),
    ("first off by one", "first=k, packets=0", "first=k + 1, packets=0"),
    ("bytes count bad extents", "ln if frames[i] is not None and ln <= 65535 else 0", "ln"),
    ("bytes count frames over 65535", "frames[i] is not None and ln <= 65535", "frames[i] is not None"),
    ("group_of one early", "group_of[i] = len(rows) - 1", "group_of[i] = max(len(rows) - 2, 0)"),
]


def result(fn, args):
    groups, group_of, n = fn(*args)
    return groups.tobytes(), group_of.tobytes(), n


@pytest.mark.parametrize("name,old,new", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_the_corpus_notices(hand, fuzz, name, old, new):
    bad = variant(groups_host, old, new, 0)
    for inp in (hand, fuzz):
        for s, p in OPTIONS:
            try:
                if result(bad, inp.args(s, p)) != result(groups_host, inp.args(s, p)):
                    return
            except Exception:  # noqa: BLE001 - a variant that raises is a detected fault
                return
    pytest.fail(f"{name}: no corpus input tells `{new}` from `{old}` in groups_host")
