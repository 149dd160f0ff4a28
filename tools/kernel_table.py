#!/usr/bin/env python3
"""Per-kernel resources and instruction mix of HIP sources, from the gfx950
assembly (hipcc --cuda-device-only -S -Rpass-analysis=kernel-resource-usage, the
library's flags): one tab-separated row per kernel with VGPRs, SGPRs, scratch
bytes per lane, static LDS bytes, occupancy (waves per SIMD), the instruction
total and the counts of global loads / stores, flat accesses, LDS reads /
writes, scalar loads, barriers and waits, and a digest of the instruction
stream with register numbers and labels blanked (equal digests: the same
code up to register naming). Rows are sorted by demangled name, so the tables
of two trees can be compared with diff.
usage: python tools/kernel_table.py [-D...] nex_amd/csrc/nexg_build.hip [more.hip ...] > table.tsv"""
import hashlib
import re
import subprocess
import sys

HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function"]
MIX = [("global_load", r"global_load_"), ("global_store", r"global_store_"), ("flat", r"flat_(load|store)_"),
       ("lds_read", r"ds_read"), ("lds_write", r"ds_write"), ("scalar_load", r"s_(buffer_)?load_"),
       ("barrier", r"s_barrier"), ("waitcnt", r"s_waitcnt")]
REMARKS = [("vgprs", "VGPRs"), ("sgprs", "TotalSGPRs"), ("scratch", "ScratchSize [bytes/lane]"), ("lds", "LDS Size [bytes/block]"),
           ("occupancy", "Occupancy [waves/SIMD]")]


def kernels(src, defs):
    p = subprocess.run([HIPCC] + FLAGS + defs + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                                                  "-o", "-", src], capture_output=True, text=True, check=True)
    res, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s*([^:]+): (\d+))", line)
        if m and m.group(1):
            cur = res.setdefault(m.group(1), {})
        elif m and cur is not None:
            cur[m.group(2).strip()] = int(m.group(3))
    asm = p.stdout
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    if not names:  # a source without kernels (c++filt without arguments would wait on stdin)
        return
    demangled = subprocess.run(["c++filt"] + names, capture_output=True, text=True,
                               check=True).stdout.splitlines()
    for name, dm in zip(names, demangled):
        start = asm.index("\n" + name + ":")
        body = asm[start:asm.index(".Lfunc_end", start)].splitlines()[2:]
        ins = [l.split(";")[0].strip() for l in body]
        ins = [l for l in ins if l and not l.startswith(".") and not l.endswith(":")]
        blank = [re.sub(r"\b[vsa]\[?\d+(:\d+)?\]?|\.LBB\w+", "R", l) for l in ins]
        row = {k: res[name].get(label, -1) for k, label in REMARKS}
        row.update(total=len(ins), digest=hashlib.sha1("\n".join(blank).encode()).hexdigest()[:10])
        row.update({k: sum(bool(re.match(rx, l)) for l in ins) for k, rx in MIX})
        yield re.sub(r"^void nexg::|\(.*\)$", "", dm), row


def main():
    defs = [a for a in sys.argv[1:] if a.startswith("-D")]
    rows = sorted(kv for src in sys.argv[1:] if not src.startswith("-D") for kv in kernels(src, defs))
    cols = [k for k, _ in REMARKS] + ["total"] + [k for k, _ in MIX] + ["digest"]
    print("\t".join(["kernel"] + cols))
    for name, row in rows:
        print("\t".join([name] + [str(row[c]) for c in cols]))


if __name__ == "__main__":
    main()
