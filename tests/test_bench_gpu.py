"""-m gpu: a plain `python bench.py` run does only what its headline needs (no roofline leg, no secondary configs, no CPU
baseline) and `--dump-outputs DIR` writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "8", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["metric"] == "unet_train_steps_per_sec_bs256" and j["unit"] == "bs256-steps/s" and j["higher_is_better"] is True
    assert j["dtype"] == "bf16" and j["steps"] == 3 and j["step_ms"]["n"] == 3 and j["ms_per_step"] > 0 and j["value"] > 0
    assert not {"roofline", "kernel_families", "secondary", "cpu_baseline"} & set(j), sorted(j)
    files = {p.name: np.load(p) for p in out.iterdir()}
    assert set(files) == {"loss.npy", "grad_norm.npy", "nan_flag.npy", "grads_sample.npy", "params_sample.npy"}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in files.values())
    assert sum(p.stat().st_size for p in out.iterdir()) < 64 << 20
    assert float(files["loss.npy"][0]) == pytest.approx(j["final_loss"]) and int(files["nan_flag.npy"][0]) == j["nan_flag"] == 0
    assert files["params_sample.npy"].shape == files["grads_sample.npy"].shape and files["params_sample.npy"].size > 1 << 20
