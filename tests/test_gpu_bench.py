"""bench.py as a plain run (no --full): the headline line and, with --dump-outputs, the factor of the last timed step, which is the
reference's L."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def run_bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_dumps_the_factor_of_its_last_step(tmp_path, golden):
    out = tmp_path / "dump"
    line = run_bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out))
    assert (line["steps"], line["warmup"], line["unit"], line["higher_is_better"], line["dtype"]) == (3, 1, "GF/s", True, "f64")
    assert line["config"]["factor_info"] == [0, 0] and line["ms_per_step"] > 0
    assert abs(line["value"] - line["config"]["F_ref_flops"] / line["ms_per_step"] * 1e-6) <= 1e-3 * line["value"]
    assert "roofline" not in line and "cpu_baseline" not in line and "large_front" not in line
    assert os.listdir(out) == ["L.npy"]
    L = np.load(out / "L.npy")
    g = golden("lapl_3375x3375")
    n = g["n"]
    assert L.dtype == np.float64 and L.shape == (n * (n + 1) // 2,)
    assert np.abs(L - g["L"][np.tril_indices(n)]).max() <= 1e-12


@pytest.mark.gpu
def test_plain_run_dumps_the_fp32_factor(tmp_path, golden):
    out = tmp_path / "dump"
    line = run_bench("--case", "lapl_400x400", "--precision", "mixed", "--steps", "2", "--warmup", "1", "--dump-outputs", str(out))
    assert line["dtype"] == "f32 factor + f64 iterative refinement" and line["steps"] == 2
    L = np.load(out / "L.npy")
    g = golden("lapl_400x400")
    Lg = g["L"][np.tril_indices(g["n"])]
    assert L.dtype == np.float32 and L.shape == Lg.shape
    assert np.abs(L - Lg).max() <= 2e-5 * np.abs(Lg).max()  # an fp32 factor of an fp64-representable matrix
