"""The benchmark's command line on the GPU, at a small size: a plain run prints the headline alone and
`--dump-outputs` writes the last timed step's results; everything else the line can carry waits for `--full`."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

FULL_ONLY = ("roofline", "splats", "hbm_model", "default_precision_mode", "f32_grade_fit", "dropin_op", "dropin_depth_loss",
             "psnr_vs_ref", "pmc", "sclk_mhz", "cpu_baseline", "reduce_us_per_view", "binning_us_per_view")


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_plain_bench_run_prints_the_headline_and_dumps(cuda, tmp_path):
    n, V, R, steps = 3000, 4, 96, 3
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--gaussians", str(n), "--views", str(V), "--res", str(R), "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=100, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = lines[0]
    assert d["unit"] == "Mpixels/sec" and d["higher_is_better"] is True and d["dtype"].startswith("f32")
    assert d["steps"] == steps and d["warmup"] == 1 and d["n_gpus"] == 1 and d["ms_per_step"] > 0
    # value and ms_per_step are the same measurement (each rounded on the line)
    assert abs(d["value"] - V * R * R / (d["ms_per_step"] * 1e3)) <= 0.01 * d["value"] + 0.01
    assert not [k for k in FULL_ONLY if k in d]
    names = ["loss", "means", "scales_raw", "opacities_raw", "colors_raw"]
    names += ["grad_" + k for k in names[1:]]
    assert sorted(os.listdir(tmp_path / "out")) == sorted(k + ".npy" for k in names)
    got = {k: np.load(tmp_path / "out" / (k + ".npy")) for k in names}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert got["loss"][0] == np.float32(d["loss"]) and got["means"].shape == (n, 3) and got["grad_opacities_raw"].shape == (n,)
    assert all(np.abs(got[k]).max() > 0 for k in names)
