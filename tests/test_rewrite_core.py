"""CPU: the per-frame core of nexg_rewrite_batch (nex_amd/csrc/rewrite_core.hpp)
as a stand-alone host program with AddressSanitizer + UBSan
(tests/native/rewrite_fuzz), and the resource report of the two kernel
instances.

The program runs the core (the very code k_rewrite runs on the device) over
the corpus of tests/rewrite_frames.py under every action and both checksum
modes, each frame at each of the 16 byte phases in an allocation that covers
exactly the 16-B blocks overlapping the frame, and over every truncation of
the corpus frames to 0..120 B. Bytes and rows must equal the expectations
written beside them (rewrite_ref for the corpus, rewrite_host for the
truncations); a read or write outside a frame's blocks is a sanitizer report."""
import os
import re
import struct
import subprocess

from nex_amd import abi
from nex_amd.rewrite import rewrite_host
from tests import rewrite_frames as rf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "nex_amd", "csrc")
ALL_PHASES = 0xFFFF
TRUNC_ACTIONS = ("everything 4", "everything 6", "nat66 + ports", "router: macs + dec_ttl 1")


def write_case(f, acts, incremental, flags, k, phases, frames, index, want_frames, want_rows):
    f.write(bytes(rf.to_set(acts, incremental).to_c()))
    f.write(struct.pack("<IIII", flags, k, phases, len(frames)))
    for fr, a, wf, row in zip(frames, index, want_frames, want_rows):
        assert len(wf) == len(fr)
        f.write(struct.pack("<II", len(fr), a) + fr + wf + row.tobytes())


def corpus_file(path):
    c = rf.corpus()
    n = 0
    with open(path, "wb") as f:
        for incremental in (False, True):
            modes = [(0, 0, half) for half in (c.fixed, c.garbage)]
            modes += [(abi.PARSE_FROM_IP, k, half) for k in rf.RAW_OFFSETS for half in rf.raw_ip(k)]
            for flags, k, frames in modes:
                ref = rf.ref_all(frames, incremental, flags, k)
                for first, acts in rf.action_chunks():
                    for j in range(len(acts)):
                        out, rows = ref[first + j]
                        # raw-IP variants: the same code at four phases only
                        write_case(f, acts, incremental, flags, k, ALL_PHASES if not flags else 0x8083, frames,
                                   [j] * len(frames), out, rows)
                        n += len(frames)
            # every truncation of every corpus frame to 0..120 B (the halves differ in checksum bytes only: the
            # garbage half), and the index values past the set
            cut = sorted({fr[:t] for fr in c.garbage for t in range(0, min(len(fr), 121))})
            acts = [rf.ACTIONS[rf.NAMES.index(name)] for name in TRUNC_ACTIONS]
            for j in range(len(acts)):
                out, rows = rewrite_host(cut, rf.to_set(acts, incremental), [j] * len(cut))
                write_case(f, acts, incremental, 0, 0, ALL_PHASES, cut, [j] * len(cut), out, rows)
                n += len(cut)
            index = [len(acts), abi.ACTION_NONE, 16, 200] * 2
            out, rows = rewrite_host(list(c.garbage[:8]), rf.to_set(acts, incremental), index)
            write_case(f, acts, incremental, 0, 0, ALL_PHASES, c.garbage[:8], index, out, rows)
            n += 8
    return n


def test_core_under_sanitizers_equals_the_contract(oracle, tmp_path):
    subprocess.check_call(["make", "-s", "-C", NATIVE, "-f", "rewrite_fuzz.mk", "rewrite_fuzz"])
    path = tmp_path / "rewrite_corpus.bin"
    frames = corpus_file(path)
    r = subprocess.run([os.path.join(NATIVE, "rewrite_fuzz"), str(path)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
                                UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    m = re.search(r"cases (\d+) frames (\d+) runs (\d+) mismatches 0", r.stdout)
    assert m, r.stdout
    assert int(m.group(2)) == frames and int(m.group(3)) >= 4 * frames and frames >= 50000


def test_kernels_use_no_scratch(tmp_path):
    """The resource report of nexg_rewrite.hip (the Makefile's `resources`
    target, on this file): neither instance of k_rewrite spills to scratch."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "nexg_rewrite.hip"), "-o",
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
    for instance in ("ILb0E", "ILb1E"):  # RECOMPUTE, INCREMENTAL
        found = [n for n in report if re.search(rf"\d+k_rewrite{instance}", n)]
        assert len(found) == 1, (instance, sorted(report))
        assert report[found[0]] == 0, (instance, report[found[0]])
