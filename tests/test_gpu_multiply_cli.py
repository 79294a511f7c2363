"""cholamd_mmat --check: one line "factor residual: %.3e" after the factorisation, the right-hand side as probe, the factor of the chosen precision.

Bound: that of test_gpu_multiply.test_factor_residual -- C_BE (k + 1) u || |L| |L^T| |z| ||_2 / ||A z||_2 with the golden factor L of the reference project
and the golden P A P^T, u = 2^-53 (fp64) or 2^-24 (--precision mixed: the fp32 factor)."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import ROOT, case_paths  # noqa: E402
from spd_inputs import C_BE, U32, U64  # noqa: E402

BIN = os.path.join(ROOT, "cholesky_amd", "bin", "cholamd_mmat")


@pytest.mark.parametrize("mixed", [False, True], ids=["fp64", "fp32"])
def test_cli_check_line(mixed, golden):
    import cholesky_amd as ca
    case = "lapl_400x400"
    m, o, c, b = case_paths(case)
    g = golden(case)
    plan = ca.Plan(m, o, c)
    perm = plan.perm
    z = ca.plan.read_vector(b, plan.n)
    aL = np.abs(g["L"])
    PAP = g["pmat"] + np.tril(g["pmat"], -1).T
    k = int((g["L"] != 0).sum(axis=1).max())
    bound = C_BE * (k + 1) * (U32 if mixed else U64) * np.linalg.norm(aL @ (aL.T @ np.abs(z[perm]))) / np.linalg.norm(PAP @ z[perm])
    outs = []
    for flag in (False, True):
        args = [BIN, "-i", m, "-s", o, "-c", c, "-b", b] + (["--precision", "mixed"] if mixed else []) + (["--check"] if flag else [])
        p = subprocess.run(args, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        outs.append(p.stdout)
    lines = [ln for ln in outs[1].splitlines() if ln.startswith("factor residual: ")]
    assert len(lines) == 1 and "factor residual" not in outs[0]
    assert [ln for ln in outs[1].splitlines() if not ln.startswith("factor residual")] == outs[0].splitlines()     # nothing else changes
    rel = float(lines[0].split(": ")[1])
    assert lines[0] == "factor residual: %.3e" % rel
    print(f"cli {'fp32' if mixed else 'fp64'}: {lines[0]} (bound {bound:.3e})")
    assert 0.0 <= rel <= bound
    # without a right-hand side there is no probe
    p = subprocess.run([BIN, "-i", m, "-s", o, "-c", c, "--check"], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "--check" in p.stderr
