"""CPU: the per-frame core of nexg_fragment_plan / nexg_fragment_frames
(nex_amd/csrc/fragment_core.hpp) as a stand-alone host program with
AddressSanitizer + UBSan (tests/native/fragment_fuzz), and the resource report
of the kernels.

The program runs the core (the very code k_fragment_frames runs on the device,
one call per lane of a frame's group and phase of the kernel) over the corpus
of tests/fragment_frames.py under six options, each frame at each of the 16
source and 16 destination byte phases (the two frames of 65535 bytes at three
phases each way), in allocations that cover exactly the 16-B blocks
overlapping the frame and the output range and exactly the table entries the
frame may write; again with out_cap and out_first[i + 1]
cut into the middle of the frame's output, and with out_bytes[i + 1] cut into
it; frames whose extent leaves the data have no source allocation at all.
Bytes, table entries and rows must equal fragment_host's, written beside them;
a read or write outside the allocations is a sanitizer report."""
import os
import re
import struct
import subprocess

from nex_amd import abi
from nex_amd.fragment import fragment_host
from tests import fragment_frames as ff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "nex_amd", "csrc")
ALL_PHASES = 0xFFFF
#: (mtu, ignore_df, align)
OPTIONS = ((68, False, 1), (576, False, 16), (1280, True, 8), (1500, False, 1), (1500, True, 16), (9000, True, 4))


def write_case(f, mtu, ignore_df, align, sphases, dphases, frames, first_index):
    pieces, src, rows = fragment_host(frames, mtu, ignore_df)
    f.write(struct.pack("<IIIIII", mtu, abi.FRAG_IGNORE_DF if ignore_df else 0, align, sphases, dphases, len(frames)))
    for i, (fr, row) in enumerate(zip(frames, rows)):
        a, n = int(row["first"]), int(row["pieces"])
        f.write(struct.pack("<IIIII", 0 if fr is None else len(fr), fr is not None, first_index + i, a, n) + row.tobytes() +
                (fr or b""))
        for p in pieces[a:a + n]:
            f.write(struct.pack("<I", len(p)) + p)
    return len(frames), len(pieces)


def corpus_file(path):
    frames = ff.frames()
    small = [frames[i] for i in ff.small(65535)]
    large = [f for f in frames if f is not None and len(f) >= 65535]
    assert len(large) == 2
    n = runs = 0
    with open(path, "wb") as f:
        for mtu, ignore_df, align in OPTIONS:
            n += write_case(f, mtu, ignore_df, align, ALL_PHASES, ALL_PHASES, small, 0)[0]
            runs += 256 * len(small)
            n += write_case(f, mtu, ignore_df, align, 0x8081, 0x4003, large, 1000)[0]  # phases 0, 7, 15 to 0, 1, 14
            runs += 9 * len(large)
    return n, runs


def test_core_under_sanitizers_equals_fragment_host(tmp_path):
    subprocess.check_call(["make", "-s", "-C", NATIVE, "-f", "fragment_fuzz.mk", "fragment_fuzz"])
    path = tmp_path / "fragment_corpus.bin"
    frames, runs = corpus_file(path)
    r = subprocess.run([os.path.join(NATIVE, "fragment_fuzz"), str(path)], capture_output=True, text=True, timeout=1800,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
                                UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    m = re.search(r"cases (\d+) frames (\d+) runs (\d+) pieces (\d+) mismatches 0", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) == 2 * len(OPTIONS) and int(m.group(2)) == frames == len(OPTIONS) * len(ff.frames())
    # every frame with output ran uncut, most of them cut twice as well; the 8183-piece frame ran 27 times
    assert int(m.group(3)) >= runs and int(m.group(4)) >= 27 * 8183


def test_kernels_use_no_scratch(tmp_path):
    """The resource report of nexg_fragment.hip (the Makefile's `resources`
    target, on this file): none of its kernels spills to scratch."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "nexg_fragment.hip"), "-o",
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
    for kernel in ("k_fragment_plan_sum", "k_fragment_plan_write", "k_fragment_frames", "k_tile_scan"):
        found = [n for n in report if re.search(rf"\d+{kernel}", n)]
        assert len(found) == 1, (kernel, sorted(report))
        assert report[found[0]] == 0, (kernel, report[found[0]])
