"""A plain `bench.py` run (no --full) at a tiny shape: only the headline leg runs, --steps sets
the number of timed steps, and --dump-outputs writes what the last timed step returned plus
the seeded parameter sample as float32 .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_runs_headline_only_and_dumps_outputs(tmp_path):
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
           "--warmup", "1", "--batch", "2", "--num-mc", "2", "--optical", "64", "--sonar", "64",
           "--dump-outputs", str(out)]
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "triplets/s" and d["higher_is_better"] is True and d["dtype"] == "fp32"
    assert d["ms_per_step"] > 0
    assert abs(d["value"] - 2 / (d["ms_per_step"] * 1e-3)) <= 0.01 * d["value"]
    for leg in ("fp32_exact_mfma", "inference", "infer_sweep", "bf16_train", "train_sweep",
                "configs0_unimodal", "roofline", "cpu_baseline"):
        assert d[leg] is None, leg
    files = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert {"loss", "ce", "scaled_kl", "output", "predicted", "params_sample"} <= set(files)
    assert all(a.dtype == np.float32 for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 * 2 ** 20
    assert files["output"].shape == (2, 7) and files["predicted"].shape == (2,)
    assert np.array_equal(files["predicted"], files["output"].argmax(1))
    assert all(np.isfinite(a).all() for a in files.values())
    assert files["params_sample"].size == 1 << 20 and np.abs(files["params_sample"]).max() > 0
    np.testing.assert_allclose(files["loss"], files["ce"] + files["scaled_kl"], rtol=1e-5)
