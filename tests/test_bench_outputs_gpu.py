"""bench.py on the GPU, end to end on the smallest model: a plain run times the headline only and
prints one result line; --dump-outputs writes what one step of the timed path computes from the
seeded start state."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--model", "trivial",
                        "--batch_size", "8", "--no_tune", *extra], env=env, capture_output=True, text=True,
                       timeout=150)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout  # stdout carries exactly the result line
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_steps_outputs(tmp_path):
    out = tmp_path / "dump"
    res = _bench("--steps", "3", "--warmup", "3", "--dump-outputs", str(out))
    assert res["steps"] == 3 and res["warmup"] == 3 and res["dtype"] == "fp32"
    assert res["ms_per_step"] > 0 and res["unit"] == "images/sec" and res["higher_is_better"] is True
    assert abs(res["value"] - 8 * 1000.0 / res["ms_per_step"]) <= 0.01 * res["value"]
    assert not any(k.startswith("bf16_") for k in res)  # the secondary figure is --full's
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert sorted(got) == ["bn_buffers", "loss", "params"]
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    assert got["loss"].shape == (1,) and float(got["loss"][0]) > 0  # cross-entropy + weight decay
    assert got["params"].shape == (4 << 20,) and np.abs(got["params"]).max() > 0  # the sampled path
