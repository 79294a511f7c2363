"""cholamd_mmat --deterministic-solve: two runs of the program write byte-identical solution files at full precision (fp64 factor, and the mixed
path's refinement on the fp32 factor), and the solution is the reference's."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, case_paths

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "cholesky_amd", "bin", "cholamd_mmat")


@pytest.mark.parametrize("precision", ["fp64", "mixed"])
def test_cli_deterministic_solve_repeats_its_bytes(precision, tmp_path, golden):
    m, o, c, b = case_paths("lapl_400x400")
    files = []
    for run in range(2):
        sol = tmp_path / f"x{run}.txt"
        r = subprocess.run([BIN, "-i", m, "-s", o, "-c", c, "-b", b, "-o", str(sol), "--deterministic-solve", "--full-precision", "--precision", precision],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "Done solve." in r.stdout
        files.append(sol.read_bytes())
    assert files[0] == files[1] and len(files[0]) > 0
    g = golden("lapl_400x400")
    x = np.genfromtxt(str(tmp_path / "x0.txt")).reshape(-1)
    assert np.abs(x - g["x"]).max() <= 1e-10 * max(1.0, np.abs(g["x"]).max())
