"""CPU: the builders' grid sizing (nex_amd/csrc/build_core.hpp build_tile_count
and build_grid, used by every builder launch) by the stand-alone program
tests/native/build_grid_test: counts that give 0, 1, 2^32 - 1 and 2^32 tiles
and the largest count, for tiles of 64 and 256 frames. A count whose tiles do
not fit one grid must be refused with hipErrorInvalidValue, not truncated."""
import subprocess

from tests.helpers import build_native_test


def test_grid_sizing():
    r = subprocess.run([build_native_test("build_grid_test")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.split()
    assert last[0] == "ok" and int(last[1]) == 20, r.stdout  # 2 tile sizes x 10 counts
