"""CPU: the workspace layouts the launchers carve their pointers from (flow,
the select / decap_select / match_select compaction, the gather / encap /
fragment plans; nex_amd/csrc/workspace_layout.hpp) against the size formulas of
include/nexg.h, by the stand-alone program tests/native/workspace_layout_test:
equal sizes, every region aligned to its element, disjoint and in bounds, for
counts around the 256- and 1024-frame tiles up to 2^32 - 1 and 1..256 buckets.
A wrong carve would be an out-of-bounds store on the device; here it is a
failing line."""
import subprocess

from tests.helpers import build_native_test


def test_layouts_match_the_header():
    r = subprocess.run([build_native_test("workspace_layout_test")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.split()
    assert last[0] == "ok" and int(last[1]) >= 1150, r.stdout  # 10 counts x (85 flow + 30 tile-table) checks
