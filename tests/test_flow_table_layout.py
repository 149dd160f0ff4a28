"""CPU: nexg_flow_entry and the flow table's workspace as the C compiler sees
them (tests/native/cpp_flow_table_test --link, which includes include/nexg.h
and nex_amd/csrc/workspace_layout.hpp) against nex_amd/abi.py: the struct's
size and field offsets, the header's workspace helper, and FlowTableLayout's
regions (aligned to their element, inside the workspace, disjoint) over a grid
of (n_in, n_groups)."""
import ctypes
import os
import re
import subprocess

import pytest

from nex_amd import abi
from tests import flow_frames as ff
from tests import helpers

COUNTS = [0, 1, 255, 256, 257, 65793, (1 << 31) - 1]
GRID = [(a, b) for a in COUNTS for b in COUNTS]


@pytest.fixture(scope="module")
def probe():
    exe = helpers.build_native_test("cpp_flow_table_test")
    argv = [str(x) for pair in GRID for x in pair]
    r = subprocess.run([exe, "--link"] + argv, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.splitlines()


def test_the_wrappers_link(probe):
    assert probe[0].split() == ["link", "ok", "2"]


def test_entry_layout_matches_the_header(probe):
    tok = probe[1].split()
    got = dict(zip(tok[0::2], (int(x) for x in tok[1::2])))
    assert got.pop("struct") == abi.FLOW_ENTRY_DTYPE.itemsize == 64
    assert got == {n: abi.FLOW_ENTRY_DTYPE.fields[n][1] for n in abi.FLOW_ENTRY_DTYPE.names}
    assert abi.FLOW_ENTRY_DTYPE.fields["key"][0].shape == (36,)
    assert probe[2].split()[:2] == ["mixed", str(abi.FLOW_ENTRY_MIXED)]


def test_workspace_helper_matches_the_header(probe):
    lines = [l.split() for l in probe[3:] if l.startswith("workspace")]
    assert lines == [["workspace", str(a), str(b), str(abi.flow_table_workspace(a, b))] for a, b in GRID]


def test_workspace_regions(probe):
    lines = [[int(x) for x in l.split()[1:]] for l in probe[3:] if l.startswith("layout")]
    assert [tuple(l[:2]) for l in lines] == GRID
    for n_in, n_groups, positions, tiles, mark, tile_first, nbytes in lines:
        assert positions == n_in + n_groups and tiles == (positions + 255) // 256
        assert nbytes == abi.flow_table_workspace(n_in, n_groups) and nbytes % 8 == 0
        regions = sorted([(mark, 8, positions), (tile_first, 4, tiles)])
        end = 0
        for off, elem, n in regions:
            assert off % elem == 0 and off >= end, (n_in, n_groups, off)  # aligned, past the region before
            end = off + elem * n
        assert end <= nbytes, (n_in, n_groups)


def test_header_declares_and_library_exports():
    text = open(os.path.join(ff.ROOT, "include", "nexg.h")).read()
    assert re.search(r"^int nexg_flow_table_merge\(nexg_ctx\* ctx,", text, re.M)
    assert "nexg_flow_table_merge" in abi.EXPORTED_SYMBOLS and "nexg_flow_table_workspace" in abi.HEADER_INLINE
    from nex_amd import _lib
    lib = _lib.load()
    assert lib.nexg_flow_table_merge.restype is ctypes.c_int and len(lib.nexg_flow_table_merge.argtypes) == 17
    # without a context the entry refuses cleanly
    assert lib.nexg_flow_table_merge(None, None, None, None, None, 0, None, 0, 0, 0, None, 0, None, None, None, 0,
                                     None) == abi.EINVAL
