"""cholamd_mmat --lowrank FILE K [--lowrank-mode update|downdate|constraint]: the solve of -b becomes the corrected solve (e = 0), --logdet prints log det C
on a line of its own after the logdet line, and without the flag nothing changes."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import lowrank_ref as lr  # noqa: E402
import tree_inputs  # noqa: E402
from conftest import ROOT  # noqa: E402
from guarded import Guarded  # noqa: E402
from oracle import oracle as orc  # noqa: E402

BIN = os.path.join(ROOT, "cholesky_amd", "bin", "cholamd_mmat")
NAME = "lapl_400x400"


def write_array(path, V):
    """A Matrix-Market dense array file as cholamd_read_vector reads it: three header lines, then the values column by column."""
    V = np.asarray(V, dtype=np.float64).reshape(V.shape[0], -1)
    with open(path, "w") as f:
        f.write("%%%%MatrixMarket matrix array real general\n%%\n%d %d\n" % V.shape)
        f.writelines("%.17g\n" % v for v in V.T.ravel())


def run(args):
    """The program's stdout with the name of the solution file (the argument of -o) replaced by SOLUTION."""
    args = [str(a) for a in args]
    r = subprocess.run([BIN] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout.replace(args[args.index("-o") + 1], "SOLUTION")


@pytest.mark.parametrize("mode,k,nrhs", [("update", 17, 33), ("downdate", 32, 33), ("constraint", 16, 1)])
def test_cli_lowrank_solution_matches_the_library(mode, k, nrhs, tmp_path, tmp_path_factory):
    import cholesky_amd as ca
    import torch
    orc.use_own_kernels()
    S = tree_inputs.cached(tmp_path_factory, NAME)
    U, rs, B, E, Xref, _ = lr.prepare(S, NAME, lr.MODES[mode], k, nrhs)
    assert E is None                                                  # the program's e is zero
    ufile, bfile = tmp_path / "U.mtx", tmp_path / "b.mtx"
    write_array(ufile, U)
    write_array(bfile, S.rhs)
    base = ["-i", S.mtx, "-s", S.ord, "-c", S.clust, "-b", bfile, "--full-precision", "--deterministic-solve"]
    plain = run(base + ["-o", tmp_path / "x0.txt", "--logdet"])
    out = run(base + ["-o", tmp_path / "x1.txt", "--logdet", "--lowrank", ufile, k, "--lowrank-mode", mode])
    quiet = run(base + ["-o", tmp_path / "x2.txt", "--lowrank", ufile, k, "--lowrank-mode", mode])
    noflag = run(base + ["-o", tmp_path / "x3.txt"])
    # without --lowrank nothing changes; with it the only new line is "logdet C", right after the logdet line
    assert "logdet C" not in plain and quiet == noflag
    lines, plines = out.splitlines(), plain.splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("logdet C: ")]
    assert len(at) == 1 and lines[at[0] - 1].startswith("logdet: ") and lines[:at[0]] + lines[at[0] + 1:] == plines
    assert (tmp_path / "x0.txt").read_bytes() == (tmp_path / "x3.txt").read_bytes()
    assert (tmp_path / "x1.txt").read_bytes() == (tmp_path / "x2.txt").read_bytes() != (tmp_path / "x0.txt").read_bytes()
    # the library's own corrected solve under the same option: the same bits (%.17g round-trips)
    dev = ca.Device(S.plan, 0)
    a = dev.new_arena()
    dev.fill(a)
    dev.factor(a)
    dev.sync()
    assert dev.info() == (0, 0)
    dev.set_option("solve_deterministic", 1)
    low = ca.LowRank(dev, k)
    low.set(a, Guarded(S.n, k, S.n, values=U).t, mode)
    x = torch.empty(S.n, dtype=torch.float64, device="cuda")
    low.solve(a, torch.from_numpy(S.rhs.copy()).cuda(), x)
    dev.sync()
    xl, xc = x.cpu().numpy(), np.genfromtxt(str(tmp_path / "x1.txt")).reshape(-1)
    assert np.array_equal(xl, xc)
    err = lr.forward_error(S, xc, Xref[:, 0]) / rs.gate4()
    ldc = float(lines[at[0]].split()[-1])
    r5 = abs(ldc - rs.logdet_c) / rs.gate5()
    print(f"--lowrank {mode} k {k}: solution error / gate 4 = {err:.3e}, logdet C error / gate 5 = {r5:.3e}")
    assert err <= 1.0 and r5 <= 1.0 and ldc == low.logdet_c()
    low.close()


def test_cli_lowrank_refusals(tmp_path, tmp_path_factory):
    S = tree_inputs.cached(tmp_path_factory, NAME)
    ufile, bfile = tmp_path / "U.mtx", tmp_path / "b.mtx"
    write_array(ufile, lr.build_u(S, 4, lr.DOWNDATE, c=2.0))
    write_array(bfile, S.rhs)
    base = [BIN, "-i", S.mtx, "-s", S.ord, "-c", S.clust, "-b", str(bfile)]
    for extra, msg in ((["--lowrank", str(ufile), "4", "--lowrank-mode", "downdate"], "not positive definite"), (["--lowrank", str(ufile), "4", "--lowrank-mode", "sideways"], "update, downdate or constraint"),
                       (["--lowrank", str(ufile), "4", "--precision", "mixed"], "fp64"), (["--lowrank", str(ufile)], "--lowrank FILE K"), (["--lowrank", str(ufile), "5"], "missing")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
