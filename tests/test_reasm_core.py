"""CPU: the per-frame core of nexg_reasm_plan / nexg_reasm_frames
(nex_amd/csrc/reasm_core.hpp) as a stand-alone host program with
AddressSanitizer + UBSan (tests/native/reasm_fuzz, run directly: it needs no
preload), and the resource report of the kernels.

The program runs the core (the very code the kernels run on the device, one
call per lane of a frame's group and phase of the kernel) over the corpus of
tests/reasm_frames.py: every frame in an allocation that covers exactly the
16-B blocks overlapping it, every output frame in one that covers exactly the
blocks overlapping its range, at each of the 16 source and 16 destination
byte phases (3 x 3 for the 64-KiB trains and the 8183-piece train); again
with out_cap in the middle,
with out_bytes[h + 1] in the middle, and with rows[i].head naming another
output frame. Rows and bytes must equal reassemble_host's, written beside
them; a read or write outside the allocations is a sanitizer report."""
import os
import re
import struct
import subprocess

from nex_amd.reassemble import reassemble_host
from tests import reasm_frames as rf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "nex_amd", "csrc")
ALL, THREE_S, THREE_D = 0xFFFF, 0x8081, 0x4003


def write_table(f, align, sphases, dphases, frames):
    out, src, rows, _ = reassemble_host(frames, align, exact=False)
    f.write(struct.pack("<IIII", align, sphases, dphases, len(frames)))
    for fr in frames:
        f.write(struct.pack("<II", 0 if fr is None else len(fr), fr is not None) + (fr or b""))
    f.write(rows.tobytes() + struct.pack("<I", len(out)))
    for o in out:
        f.write(struct.pack("<I", len(o)) + o)
    return len(frames)


def corpus_file(path):
    n = tables = 0
    with open(path, "wb") as f:
        for k, (name, classes, frames) in enumerate(rf.cases()):
            big = any(fr is not None and len(fr) > 4200 for fr in frames)
            sp, dp = (THREE_S, THREE_D) if big else (ALL, ALL)
            n += write_table(f, (1, 16, 4, 8)[k % 4], sp, dp, frames)
            tables += 1
        n += write_table(f, 1, THREE_S, THREE_D, list(rf.long_train())[::-1])
        n += write_table(f, 16, 0x0002, 0x0200, list(rf.long_train()))
        tables += 2
    return tables, n


def test_core_under_sanitizers_equals_reassemble_host(tmp_path):
    subprocess.check_call(["make", "-s", "-C", NATIVE, "-f", "reasm_fuzz.mk", "reasm_fuzz"])
    path = tmp_path / "reasm_corpus.bin"
    tables, frames = corpus_file(path)
    r = subprocess.run([os.path.join(NATIVE, "reasm_fuzz"), str(path)], capture_output=True, text=True, timeout=1800,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
                                UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    m = re.search(r"tables (\d+) frames (\d+) runs (\d+) lies (\d+) mismatches 0", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) == tables and int(m.group(2)) == frames
    # the 8183-piece train alone ran 3 x 3 phases, whole and cut twice; every PART of it lied once per phase pair
    assert int(m.group(3)) >= 27 * 8183 and int(m.group(4)) >= 9 * 8182


def test_kernels_use_no_scratch(tmp_path):
    """The resource report of nexg_reasm.hip (the Makefile's `resources` target,
    on this file): none of its kernels spills to scratch, and the fill keeps
    the fragment fill's LDS (one FragHdr per group of its workgroup)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "nexg_reasm.hip"), "-o",
                        str(tmp_path / "res.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    scratch, lds = {}, {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m and name:
            lds[name] = int(m.group(1))
    for kernel in ("k_reasm_classify", "k_reasm_mark", "k_reasm_place", "k_reasm_rows", "k_reasm_plan_sum", "k_reasm_plan_write",
                   "k_reasm_part_out", "k_reasm_frames", "k_tile_scan", "k_compact_count", "k_compact_scatter"):
        found = [n for n in scratch if re.search(rf"\d+{kernel}", n)]
        assert found, (kernel, sorted(scratch))
        assert all(scratch[n] == 0 for n in found), (kernel, [scratch[n] for n in found])
    fill = next(n for n in lds if "k_reasm_frames" in n)
    assert lds[fill] == 16 * 168  # 16 groups x sizeof(FragHdr): what k_fragment_frames has
