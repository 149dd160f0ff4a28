"""GPU: differential sweep of the seven frame builders over the grid of
tests/builder_sweep.py: every dispatch class of the builders' launchers at
counts 1, 255, 256, 257 and 513, aligned and unaligned `out`, the stride band
edges, payload lengths around kSmallPay and up to the largest the entry
accepts, payloads at every address shift, the TCP option sets and the optional
per-frame arrays pairwise. Every frame is compared with the oracle's
single-frame builders, every gap and both guards of the output buffer are
checked (builder_sweep.compare), forms that must agree are compared frame for
frame, the largest ragged batch of each builder is parsed back on the GPU, and
the measurement library's own instances (knob settings) are built against the
same expectation in child processes.

Cases per builder: udp4 299, udp4_tuples 96, udp6 247, tcp 552, icmp 553,
arp 63, ndp_ns 38 (1848 in 54 dispatch classes; tests/test_builder_sweep.py
asserts each class at each count). No case exceeds 513 frames but the four
largest-payload ones at 257. Wall time of each test on an MI355X, forms that
must agree included: tcp 0.5 s, udp4 0.4 s, icmp 0.3 s, udp4_tuples 0.2 s,
udp6 0.2 s, arp and ndp_ns under 0.1 s, the wrapper / raw-entry test under
0.1 s; the measurement-library test 8.6 s, which is its four child processes
starting (one per setting, one after another).

No case disagreed with the oracle when this suite was written."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from nex_amd import abi
from nex_amd.engine import FrameBatch
from tests import builder_sweep as bs

pytestmark = pytest.mark.gpu

GRID = list(enumerate(bs.cases()))


def frames_of(c, buf):
    lo = bs.GUARD + c.out_shift
    return buf[lo: lo + c.count * c.out_stride].reshape(c.count, c.out_stride)[:, :bs.frame_len(c)]


def parse_back(engine, oracle, c, seed):
    """The case's frames through the GPU parse: the oracle's verdicts, and the
    checksums the builder wrote verify wherever the oracle's parse says so."""
    import torch
    inp = bs.inputs(c, seed, oracle)
    _, out = bs.launch(engine, c, inp)
    torch.cuda.synchronize()
    L = bs.frame_len(c)
    got = engine.parse_to_numpy(FrameBatch(data=out, count=c.count, stride=L), out_kind=abi.OUT_FLAGS)["flags"]
    want = oracle.parse_packed(bs.expected(oracle, c, inp).reshape(-1), stride=L)["flags"]
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (c, int(bad[0]), hex(int(got[bad[0]])), hex(int(want[bad[0]])))
    if c.builder != "arp":
        need = abi.C_L4_OK | (abi.C_IP_OK if c.family == 4 else 0)
        assert ((got & need) == need).all(), (c, int(np.nonzero((got & need) != need)[0][0]))


def sweep(engine, oracle, builder):
    mine = [(seed, c) for seed, c in GRID if c.builder == builder]
    assert mine
    for seed, c in mine:
        inp = bs.inputs(c, seed, oracle)
        want = bs.expected(oracle, c, inp)
        buf = bs.run(engine, c, inp)
        bs.compare(c, buf, want)
        for e in bs.equivalents(c):  # forms that must give the same bytes, frame for frame
            other = bs.run(engine, e, inp)
            bs.compare(e, other, want)
            assert np.array_equal(frames_of(c, buf), frames_of(e, other)), (c, e)
    ragged = [(bs.frame_len(c), seed, c) for seed, c in mine
              if c.count == 513 and c.out_shift == 0 and c.out_stride == bs.frame_len(c)]
    _, seed, c = max(ragged)
    parse_back(engine, oracle, c, seed)


def test_sweep_udp4(engine, oracle):
    sweep(engine, oracle, "udp4")


def test_sweep_udp4_tuples(engine, oracle):
    sweep(engine, oracle, "udp4_tuples")


def test_sweep_udp6(engine, oracle):
    sweep(engine, oracle, "udp6")


def test_sweep_tcp(engine, oracle):
    sweep(engine, oracle, "tcp")


def test_sweep_icmp_echo(engine, oracle):
    sweep(engine, oracle, "icmp")


def test_sweep_arp(engine, oracle):
    sweep(engine, oracle, "arp")


def test_sweep_ndp_ns(engine, oracle):
    sweep(engine, oracle, "ndp_ns")


def test_wrapper_and_raw_entry_agree(engine, oracle):
    """The cases the Engine wrappers express give the same buffer through the
    raw library entry (the sweep takes the wrapper wherever it can)."""
    for seed, c in GRID[::7]:
        if bs.wrapper_ok(c):
            inp = bs.inputs(c, seed, oracle)
            assert np.array_equal(bs.run(engine, c, inp, raw=False), bs.run(engine, c, inp, raw=True)), c


KNOBS_CHILD = r'''
import hashlib
import sys
import torch
from nex_amd import _lib
_lib.LIB_PATH = sys.argv[1]  # the -DNEXG_AB_KNOBS build: the setting is in the environment
from nex_amd.engine import Engine
from oracle import oracle
from tests import builder_sweep as bs
e = Engine(0)
for seed, c in enumerate(bs.cases()):
    if bs.knob_class(c, sys.argv[2]) is not None:
        print(seed, hashlib.sha256(bs.run(e, c, bs.inputs(c, seed, oracle)).tobytes()).hexdigest())
'''


def test_knob_instances_match_oracle(oracle):
    """The instances only the measurement library dispatches (k_build_probe for
    ICMP and at kch 3, k_build_l4's probe form for ICMP over IPv4, k_build_lane
    for TCP, the one-wave k_build_probe): one fresh process per setting builds
    the grid's probe cases; its buffers' SHA-256 must equal those of the
    oracle's frames laid out with the gaps of the class the setting selects."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "nex_amd", "libnexg_knobs.so")
    for setting in bs.KNOB_SETTINGS:
        want = {}
        for seed, c in GRID:
            cls = bs.knob_class(c, setting)
            if cls is not None:
                exp = bs.expected(oracle, c, bs.inputs(c, seed, oracle))
                want[seed] = (hashlib.sha256(bs.layout(c, exp, cls[1]).tobytes()).hexdigest(), c, cls[0])
        assert want, setting
        name, value = setting.split("=")
        r = subprocess.run([sys.executable, "-c", KNOBS_CHILD, lib, setting], cwd=root, capture_output=True, text=True,
                           timeout=240, env=dict(os.environ, **{name: value}))
        assert r.returncode == 0, (setting, r.stderr[-2000:])
        got = dict(line.split() for line in r.stdout.strip().splitlines())
        assert set(got) == {str(s) for s in want}, setting
        bad = [(c, cls) for s, (h, c, cls) in want.items() if got[str(s)] != h]
        assert not bad, (setting, len(bad), bad[:4])
