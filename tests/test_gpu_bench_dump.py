"""bench.py as every later change runs it: a plain `--gpus 1 --steps K
--warmup W` run times K steps of the headline and nothing beside it (the CPU
baselines, stream ceilings and further objects wait for --full), and
`--dump-outputs DIR` writes what the last timed step computed: here every
frame's descriptor, equal to the oracle's parse of the same generated frames."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 4096


def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path, oracle):
    from nex_amd import abi
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--frames", str(FRAMES), "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["ms_per_step"] > 0 and res["value"] > 0
    assert res["unit"] == "Mpkt/s" and res["higher_is_better"] is True and res["dtype"] == "u8"
    assert abs(res["value"] - FRAMES / res["ms_per_step"] / 1e3) <= 0.02 * res["value"]
    for key in ("cpu_baseline", "imix", "malformed", "real_traffic", "ser", "large"):
        assert key not in res, key
    assert "stream_ceilings" not in res["roofline"]

    frames = [oracle.gen_frame(abi.WL_UDP64, i) for i in range(FRAMES)]
    want = oracle.parse_frames(frames)
    names = sorted(f for f in os.listdir(tmp_path))
    assert names == sorted(n + ".npy" for n in abi.DESC_DTYPE.names + ("frame_index",)), names
    idx = np.load(tmp_path / "frame_index.npy")
    assert idx.dtype == np.float64 and (idx == np.arange(FRAMES)).all()
    for n in abi.DESC_DTYPE.names:
        got = np.load(tmp_path / (n + ".npy"))
        assert got.dtype == np.float64 and got.shape == (FRAMES,)
        assert (got == want[n].astype(np.float64)).all(), n
