"""cholamd_mmat --inverse-block DOFS.txt FILE: A^-1[S, S] of a few dofs by a sparse solve of the identity, written dense in write_matrix's format, checked
on the fixture lapl_400x400 against the CPU oracle's solves of the unit vectors at the 1e-9 scale of the fixtures' solve tests; under --precision mixed the
flag is refused in --invdiag's words; without the flag nothing changes."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import ROOT, case_paths  # noqa: E402
from oracle import oracle as orc  # noqa: E402

BIN = os.path.join(ROOT, "cholesky_amd", "bin", "cholamd_mmat")
NAME = "lapl_400x400"
DOFS = [0, 57, 211, 399]


def read_block(path, m):
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0].startswith("%%MatrixMarket matrix coordinate real")
    assert lines[1].split() == [str(m), str(m), str(m * m)]
    Z = np.full((m, m), np.nan)
    for k, ln in enumerate(lines[2:]):
        i, j, v = ln.split()
        assert (int(i) - 1, int(j) - 1) == divmod(k, m), "row by row, 1-based"
        Z[int(i) - 1, int(j) - 1] = float(v)
    assert len(lines) == 2 + m * m
    return Z


def test_cli_inverse_block_matches_the_oracle(tmp_path):
    m, o, c, _ = case_paths(NAME)
    orc.use_own_kernels()
    O = orc.Oracle(m, o, c)
    O.factor()
    want = np.empty((len(DOFS), len(DOFS)))
    for j, dof in enumerate(DOFS):
        e = np.zeros(400)
        e[dof] = 1.0
        want[:, j] = O.solve(e)[DOFS]
    dofs = tmp_path / "dofs.txt"
    dofs.write_text("".join(f"{d}\n" for d in DOFS))
    base = [BIN, "-i", m, "-s", o, "-c", c]
    for extra, gate in ((["--full-precision"], 1e-9), ([], 1e-7)):     # (%0.8g keeps eight digits)
        out = tmp_path / f"zss{len(extra)}.mtx"
        r = subprocess.run(base + ["--inverse-block", str(dofs), str(out)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert f"Saving inverse block (4 dofs) to: {out}" in r.stdout
        Z = read_block(out, len(DOFS))
        err = float(np.abs(Z - want).max())
        print(f"--inverse-block {extra}: |Z - oracle|_max = {err:.3e} (gate {gate * max(1.0, np.abs(want).max()):.3e})")
        assert err <= gate * max(1.0, float(np.abs(want).max()))
        if extra:
            assert np.abs(Z - Z.T).max() <= 2e-9 * max(1.0, float(np.abs(want).max()))
    plain = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and plain.stdout == r.stdout.replace(f"Saving inverse block (4 dofs) to: {out}\n", "")
    # refusals: the fp32 factor, a dof outside the matrix, a duplicate, an empty list, a missing file name
    r = subprocess.run(base + ["--inverse-block", str(dofs), str(out), "--precision", "mixed"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--inverse-block needs the fp64 factor (--precision fp64)" in r.stderr
    for text, word in (("3\n7\n400\n3\n", "[2] = 400 is not a dof"), ("", "no dof")):     # (the empty list is refused before any device work)
        bad = tmp_path / "bad.txt"
        bad.write_text(text)
        r = subprocess.run(base + ["--inverse-block", str(bad), str(tmp_path / "never.mtx")], capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and word in r.stderr and not (tmp_path / "never.mtx").exists(), (text, r.stderr)
    r = subprocess.run(base + ["--inverse-block", str(dofs)], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--inverse-block DOFS.txt FILE" in r.stderr
