"""cholamd_mmat --pcg: the solve of -b through cholamd_solve_pcg (fp64 factor) / cholamd_solve_pcg_f32 (--precision mixed).  The solution is held to the
bound of a converged column (tests/test_gpu_pcg.py), ||x - x_ref|| / ||x_ref|| <= kappa_2(A) ||b - A x|| / ||b|| with the residual formed here in long
double -- against the golden x, which is a computed solution too, with the sum of the two residuals; the program reports its own residual on stderr, and says nothing new without the flag."""
import os
import re
import subprocess

import numpy as np
import pytest

import pcg_ref as pr
from conftest import ROOT, case_paths
from spd_inputs import _read_coo

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "cholesky_amd", "bin", "cholamd_mmat")
CASE = "lapl_400x400"


def run_cli(tmp_path, precision, flag):
    m, o, c, b = case_paths(CASE)
    sol = tmp_path / f"x_{precision}_{int(flag)}.txt"
    r = subprocess.run([BIN, "-i", m, "-s", o, "-c", c, "-b", b, "-o", str(sol), "--full-precision", "--precision", precision] + (["--pcg"] if flag else []),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "Done solve." in r.stdout
    return r, np.genfromtxt(str(sol)).reshape(-1)


@pytest.mark.parametrize("precision", ["fp64", "mixed"])
def test_cli_pcg(precision, tmp_path, golden):
    import cholesky_amd as ca
    m, _, _, bfile = case_paths(CASE)
    n, lo, hi, val = _read_coo(m)
    A = np.zeros((n, n))
    A[lo, hi] = val
    A[hi, lo] = val
    b = ca.plan.read_vector(bfile, n)
    gx = golden(CASE)["x"]
    r, x = run_cli(tmp_path, precision, True)
    line = re.search(r"^\[cholamd\] pcg: (\d+) iterations, \|\|b - A x\|\| / \|\|b\|\| = (\S+)$", r.stderr, re.M)
    assert line, r.stderr
    iters, rel = int(line.group(1)), float(line.group(2))
    assert iters <= 30 and rel < 1e-12  # (1e-14 is the program's target; whether fp64 reaches it is not this test's business)
    mine = pr.relres_ld(A, x, b)
    w = np.linalg.eigvalsh(A)
    err = np.linalg.norm(x - gx) / np.linalg.norm(gx)
    print(f"{precision}: {iters} iterations, reported {rel:.3e}, long double {mine:.3e}, error against the golden x {err:.3e}, kappa {w[-1] / w[0]:.1f}")
    # the golden x is itself a computed solution (its own residual is ~1e-14): both residuals bound the distance of the two
    assert err <= w[-1] / w[0] * (mine + pr.relres_ld(A, gx, b)), (err, mine)
    # without the flag: the same standard output, no new line on stderr
    r0, x0 = run_cli(tmp_path, precision, False)
    assert "] pcg:" not in r0.stderr and "] pcg:" not in r0.stdout
    assert r0.stdout.replace("_0.txt", "_1.txt") == r.stdout
    assert np.abs(x0 - gx).max() <= 1e-10 * max(1.0, np.abs(gx).max())
