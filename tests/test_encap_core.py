"""CPU: the per-frame core of nexg_encap_plan / nexg_encap_frames
(nex_amd/csrc/encap_core.hpp) as a stand-alone host program with
AddressSanitizer + UBSan (tests/native/encap_fuzz), and the resource report of
the kernels.

The program runs the core (the very code k_encap_frames runs on the device,
one call per lane of a frame's group) over the corpus of tests/encap_frames.py
under every spec, each frame at each of the 16 source and 16 destination byte
phases (the two 65-KB frames at each spec's length limit at three phases each
way: the 1500-B frames take the long frames' loop at all 256), in allocations that cover exactly the 16-B blocks overlapping the
inner frame and the output range, and again with out_cap in the middle of the
frame; frames whose extent leaves the data have no source allocation at all.
Bytes and rows must equal the expectations written beside them (the
reference of tests/encap_frames.py); a read or write outside the blocks is a
sanitizer report."""
import os
import re
import struct
import subprocess

import numpy as np

from nex_amd import abi
from tests import encap_frames as ef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "nex_amd", "csrc")
ALL_PHASES = 0xFFFF


def write_case(f, tunnels, sphases, dphases, frames, index, hashes, first, want_frames, want_rows):
    f.write(bytes(tunnels.to_c()))
    f.write(struct.pack("<III", sphases, dphases, len(frames)))
    for k, (fr, t, wf, row) in enumerate(zip(frames, index, want_frames, want_rows)):
        f.write(struct.pack("<IIIIII", 0 if fr is None else len(fr), t, first + k, int(hashes[k]), len(wf), fr is not None) +
                (fr or b"") + wf + row.tobytes())


def corpus_file(oracle, path):
    inner = list(ef.small_inner())
    hashes = ef.hashes_for(len(inner))
    n = runs = 0
    with open(path, "wb") as f:
        for tunnels, numbers in ef.spec_sets():
            for j, k in enumerate(numbers):
                index = [j] * len(inner)
                # the reference numbers frames from 0: the table index travels with each frame
                out, rows = ef.ref_all(oracle, inner, tunnels, index, hashes)
                write_case(f, tunnels, ALL_PHASES, ALL_PHASES, inner, index, hashes, 0, out, rows)
                n += len(inner)
                runs += 256 * len(inner)
                # the frames at the spec's length limit: three phases each way (0, 7, 15 to 0, 1, 14)
                big = ef.limit_inner(ef.specs()[k])
                out, rows = ef.ref_all(oracle, big, tunnels, [j, j], [9, 10])
                write_case(f, tunnels, 0x8081, 0x4003, big, [j, j], [9, 10], 0, out, rows)
                n += 2
                runs += 9 * 2
            # extents that leave the data (no source bytes at all), under every tunnel number and past the set: the
            # output is given 0..15 bytes of room all the same, which must come out zero without a source read
            which = list(range(len(numbers))) + [len(numbers), abi.TUNNEL_NONE, 16, 200]
            gone = [None] * len(which)
            out, rows = ef.ref_all(oracle, gone, tunnels, which, hashes[:len(which)])
            write_case(f, tunnels, ALL_PHASES, ALL_PHASES, gone, which, hashes[:len(which)], 0, out, rows)
            n += len(which)
            # indices past the set: pass-through
            past = [len(numbers), abi.TUNNEL_NONE, 16, 200] * 4
            out, rows = ef.ref_all(oracle, inner[:16], tunnels, past, hashes[:16])
            write_case(f, tunnels, ALL_PHASES, 0x0F0F, inner[:16], past, hashes[:16], 0, out, rows)
            n += 16
    return n


def test_core_under_sanitizers_equals_the_reference(oracle, tmp_path):
    subprocess.check_call(["make", "-s", "-C", NATIVE, "-f", "encap_fuzz.mk", "encap_fuzz"])
    path = tmp_path / "encap_corpus.bin"
    frames = corpus_file(oracle, path)
    r = subprocess.run([os.path.join(NATIVE, "encap_fuzz"), str(path)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
                                UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    m = re.search(r"cases (\d+) frames (\d+) runs (\d+) mismatches 0", r.stdout)
    assert m, r.stdout
    assert int(m.group(2)) == frames and int(m.group(3)) >= 256 * 24 * len(ef.small_inner()) and frames >= 1980


def test_kernels_use_no_scratch(tmp_path):
    """The resource report of nexg_encap.hip (the Makefile's `resources`
    target, on this file): none of its kernels spills to scratch."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "nexg_encap.hip"), "-o",
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
    for kernel in ("k_encap_plan_sum", "k_encap_plan_write", "k_encap_frames", "k_tile_scan"):
        found = [n for n in report if re.search(rf"\d+{kernel}", n)]
        assert len(found) == 1, (kernel, sorted(report))
        assert report[found[0]] == 0, (kernel, report[found[0]])
