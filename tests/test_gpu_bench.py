"""bench.py as it is run for every change: a plain run prints the headline line only, `--dump-outputs DIR` writes what
the last timed step computed, and two runs with the same arguments compute from the same inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMPED = {"y_real", "y_imag", "x_grad_real", "x_grad_imag", "grad_log_sigma2", "grad_weight_real", "grad_weight_imag",
          "grad_bias_real", "grad_bias_imag", "kl"}


def _run(out_dir, batch=1024, steps=3):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR", "TORCHELASTIC_RUN_ID", "GROUP_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--batch", str(batch), "--dump-outputs", str(out_dir)],
                       env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_run_and_dumped_outputs(tmp_path):
    B, steps = 1024, 3
    line = _run(tmp_path / "a", B, steps)
    assert line["metric"] == "Cplx-samples/sec fwd+bwd (CplxLinear-4096 + VD)" and line["unit"] == "samples/s"
    assert line["higher_is_better"] is True and line["dtype"] == "bf16" and line["steps"] == steps
    assert line["ms_per_step"] > 0 and abs(line["value"] - B / (line["ms_per_step"] * 1e-3)) < 1e-3 * line["value"]
    # what moved behind --full is not measured in a plain run
    for k in ("roofline", "hbm_kernels_GBps", "cpu_baseline", "cfg2_linear", "conv_cfg3", "dp_projection"):
        assert k not in line, k
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert set(a) == DUMPED
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["y_real"].shape == (1 << 20,) and a["grad_log_sigma2"].shape == (1 << 20,)    # seeded samples
    assert a["grad_bias_real"].shape == (4096,) and a["kl"].shape == ()
    assert abs(float(a["kl"]) - line["kl"]) <= 1e-3 + 1e-6 * abs(line["kl"])
    assert np.abs(a["y_real"]).max() > 0 and np.abs(a["grad_weight_real"]).max() > 0
    # same arguments, same inputs: a second run computes the same step (up to the summation order of a reduction)
    _run(tmp_path / "b", B, steps)
    for k, v in a.items():
        w = np.load(tmp_path / "b" / (k + ".npy"))
        np.testing.assert_allclose(w, v, rtol=1e-2, atol=1e-3 * max(float(np.abs(v).max()), 1e-30), err_msg=k)
