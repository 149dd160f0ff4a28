"""CPU: nexg_reasm_plan's workspace. workspace_layout.hpp's ReasmPlanLayout
against include/nexg.h's nexg_reasm_plan_workspace through a native program of
its own (tests/native/reasm_layout_test.cpp: regions aligned, disjoint and in
bounds, counts around 256 and 1024 up to 2^32 - 1), and both against
nex_amd.abi's restatement."""
import os
import re
import subprocess

from nex_amd import abi

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")


def test_layout_equals_the_header_and_abi():
    subprocess.check_call(["make", "-s", "-C", NATIVE, "-f", "reasm_fuzz.mk", "reasm_layout_test"])
    r = subprocess.run([os.path.join(NATIVE, "reasm_layout_test")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout[-2000:]
    sizes = {int(c): int(b) for c, b in re.findall(r"^bytes (\d+) (\d+)$", r.stdout, re.M)}
    assert {0, 1, 255, 256, 257, 1023, 1024, 1025, 0xFFFFFFFF} <= set(sizes) and len(sizes) >= 20
    for count, nbytes in sizes.items():
        assert abi.reasm_plan_workspace(count) == nbytes, count
        assert nbytes % 4 == 0 and nbytes >= abi.flow_sort_workspace(count) + 68 * count  # 56 + three u32 per frame
    m = re.search(r"^ok (\d+)$", r.stdout, re.M)
    assert m and int(m.group(1)) > 40 * len(sizes)
    assert abi.reasm_held_workspace(1000) == abi.select_workspace(1000)
