"""CPU: the per-frame core of nexg_match_batch (nex_amd/csrc/match_core.hpp)
as a stand-alone host program with AddressSanitizer + UBSan
(tests/native/match_fuzz), and the resource report of the three kernels.

The program runs the core (the code k_match runs on the device, over windows
built byte by byte instead of from registers) over the whole corpus of
tests/match_frames.py, each frame alone in a heap block that ends at its last
byte, and over random regions flush against the end of their allocation. Its
rows must equal the rows nex_amd.match.match_rows_host gives and a naive
memcmp loop's; a read outside a frame is a sanitizer report."""
import os
import re
import struct
import subprocess

from tests import match_frames as mf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "nex_amd", "csrc")


def corpus_file(oracle, path):
    frames = 0
    with open(path, "wb") as f:
        for c in mf.cases():
            recs, rows = mf.expected(oracle, c)
            f.write(bytes(c.pset.to_c()))
            f.write(struct.pack("<I", len(c.frames)))
            for fr, r, row in zip(c.frames, recs, rows):
                payload = int(r["payload_off"]) | int(r["payload_len"]) << 16
                f.write(struct.pack("<III", len(fr), int(r["flags"]), payload) + fr + row.tobytes())
                frames += 1
    return frames


def test_core_under_sanitizers_equals_the_contract(oracle, tmp_path):
    subprocess.check_call(["make", "-s", "-C", NATIVE, "-f", "match_fuzz.mk", "match_fuzz"])
    path = tmp_path / "match_corpus.bin"
    frames = corpus_file(oracle, path)
    r = subprocess.run([os.path.join(NATIVE, "match_fuzz"), str(path)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
                                UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    m = re.search(r"cases (\d+) frames (\d+) fuzzed (\d+) mismatches 0", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) == len(mf.cases()) and int(m.group(2)) == frames and int(m.group(3)) >= 4000


def test_kernels_use_no_scratch(tmp_path):
    """The resource report of nexg_match.hip (the Makefile's `resources`
    target, on this file): no kernel of it spills to scratch."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "nexg_match.hip"), "-o",
                        str(tmp_path / "res.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    report = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            report[name] = int(m.group(1))
    for kernel in ("k_match", "k_match_count", "k_match_scatter"):
        found = [n for n in report if re.search(rf"\d{kernel}E", n)]
        assert len(found) == 1, (kernel, sorted(report))
        assert report[found[0]] == 0, (kernel, report[found[0]])
