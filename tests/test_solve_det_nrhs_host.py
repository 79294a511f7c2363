"""Host restatement of the deterministic BLOCK solve (cholamd_plan_solve_det_host_nrhs, option solve_deterministic_block of the device): the step lists
of both sweeps walked over a host arena on chunks of 32 columns, every gather with the block kernel's own partition of its sources (chol_muln_wave,
chol_muln_elem) -- no device needed.

Inputs: those of tests/test_solve_det_host.py (the four fixtures and six trees; its Input class and its cache, so every reference is computed once): the
arena holds the dense fp64 Cholesky factor of P A P^T on the stored positions of the lower triangle and NaN everywhere else.  Column 0 of B is the input's
own b; the other columns are seeded normal columns scaled by the equilibration s = sqrt(diag A), as that file scales its right-hand sides.

Gates (none measured from the code under test) -- those of test_host_solve_matches_the_oracle, per column:
  * the fixtures: |x - x_ref|_max <= 1e-10 max(1, |x_ref|_max); the trees: SPD.forward_error(x, x_ref) <= SPD.tol_forward() = C_FE (k + 1) u kappa.
    x_ref of column 0 is the golden x (fixtures) or the oracle's x and the tree's x_ref (trees); of the other columns a dense numpy solve of the input's
    matrix with one correction from a long-double residual.
  * bit for bit: BACKWARD of FORWARD is the solve; a column alone, at another position of the block and beside a NaN column has the same bits; NaN in the
    upper triangles and the unstored rows of the arena changes nothing."""
import numpy as np
import pytest

import multiply_ref as mr
from test_solve_det_host import FWD, BWD, NAMES, environment, inputs  # noqa: F401  (the fixtures and the shared input cache)

NRHS = [1, 5, 33]
KMAX = max(NRHS)
_BLOCKS = {}


def block(I):
    """(A in original dof order, B with KMAX columns, its reference solution), once per input."""
    if I.name not in _BLOCKS:
        P = I.plan
        if I.S is not None:
            A = np.asarray(I.S.A, dtype=np.float64)
        else:
            A = np.empty_like(I.PAP)
            A[np.ix_(I.perm, I.perm)] = I.PAP
        B = I.s[:, None] * np.random.default_rng(77).standard_normal((P.n, KMAX))
        B[:, 0] = I.b
        X = np.linalg.solve(A, B)
        R = (B.astype(np.longdouble) - A.astype(np.longdouble) @ X.astype(np.longdouble)).astype(np.float64)
        X = X + np.linalg.solve(A, R)
        B.setflags(write=False)
        X.setflags(write=False)
        _BLOCKS[I.name] = (A, B, X)
    return _BLOCKS[I.name]


def column_gate(I, x, ref, tag):
    assert np.isfinite(x).all(), tag
    if I.S is None:
        err, gate = float(np.abs(x - ref).max()), 1e-10 * max(1.0, float(np.abs(ref).max()))
    else:
        err, gate = I.S.forward_error(x, ref), I.S.tol_forward()
    print(f"{tag}: error {err:.3e} (gate {gate:.3e})")
    assert err <= gate, tag


@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("name", NAMES)
def test_every_column_matches_its_reference(name, nrhs, inputs):
    I = inputs(name)
    P = I.plan
    _, B, Xref = block(I)
    X = P.solve_det_host_nrhs(I.arena, -1, B[:, :nrhs], ldb=P.n + 3, ldx=P.n + 2)     # (the wrapper checks that the rows n .. ldx - 1 stay untouched)
    assert X.shape == (P.n, nrhs)
    column_gate(I, X[:, 0], I.xo, f"{name} nrhs={nrhs} column 0 against the oracle")
    if I.S is not None:
        column_gate(I, X[:, 0], I.S.x_ref, f"{name} nrhs={nrhs} column 0 against the tree's x_ref")
    for j in range(nrhs):
        column_gate(I, X[:, j], Xref[:, j], f"{name} nrhs={nrhs} column {j} against the dense solve")
    # the halves compose to the solve, bit for bit; in place gives the same bits
    Y = P.solve_det_host_nrhs(I.arena, FWD, B[:, :nrhs])
    assert np.array_equal(P.solve_det_host_nrhs(I.arena, BWD, Y), X)
    W = np.asfortranarray(B[:, :nrhs].copy())
    assert P.L.cholamd_plan_solve_det_host_nrhs(P.h, I.arena.ctypes.data, -1, W.ctypes.data, P.n, W.ctypes.data, P.n, nrhs) == 0
    assert np.array_equal(W, X)


@pytest.mark.parametrize("name", NAMES)
def test_columns_are_independent(name, inputs):
    """(b): a column alone, at another position (another chunk, the other half of the tile) and beside a NaN column -- the same bits, in every sweep."""
    I = inputs(name)
    P = I.plan
    _, B, _ = block(I)
    for which in (FWD, BWD, -1):
        X = P.solve_det_host_nrhs(I.arena, which, B)
        assert np.isfinite(X).all()
        for j in (0, 4, 20, 32):
            assert np.array_equal(P.solve_det_host_nrhs(I.arena, which, B[:, j:j + 1])[:, 0], X[:, j]), (which, j, "alone")
        order = np.roll(np.arange(KMAX), 13)                       # column j goes to position (j + 13) mod 33: chunks and half-tiles change
        Xp = P.solve_det_host_nrhs(I.arena, which, B[:, order])
        assert np.array_equal(Xp, X[:, order]), (which, "permuted")
        Bn = B.copy()
        Bn[:, 7] = np.nan
        Bn[3, 32] = np.nan
        Xn = P.solve_det_host_nrhs(I.arena, which, Bn)
        keep = [j for j in range(KMAX) if j not in (7, 32)]
        assert np.isnan(Xn[:, 7]).any() and np.array_equal(Xn[:, keep], X[:, keep]), (which, "a NaN column beside it")


@pytest.mark.parametrize("name", ["lapl_400x400", "tree_over", "tree_skew", "tree_single"])
def test_nan_outside_the_factor_does_not_reach_x(name, inputs):
    """Upper triangles, padding rows and tiles without storage as zeros and as NaN: the same bits."""
    I = inputs(name)
    P = I.plan
    _, B, _ = block(I)
    clean = mr.arena_from_lower(P, I.Ld, fill=0.0)
    assert np.isnan(I.arena).any() and not np.isnan(clean).any()
    for which in (FWD, BWD, -1):
        a, b = P.solve_det_host_nrhs(clean, which, B), P.solve_det_host_nrhs(I.arena, which, B)
        assert np.isfinite(b).all() and np.array_equal(a, b), (name, which)


def test_bad_arguments_are_refused(inputs):
    I = inputs("lapl_9x9")
    P = I.plan
    n, k = P.n, 3
    B, X = np.ones((k, n)), np.full((k, n), -7.0)                  # row j = column j, leading dimension n
    f = P.L.cholamd_plan_solve_det_host_nrhs
    ar, b, x = I.arena.ctypes.data, B.ctypes.data, X.ctypes.data
    for which in (2, -2):
        assert f(P.h, ar, which, b, n, x, n, k) == -4
        assert "which" in P.L.cholamd_last_error().decode()
    assert f(None, ar, 0, b, n, x, n, k) == -4
    assert f(P.h, None, 0, b, n, x, n, k) == -4
    assert f(P.h, ar, 0, None, n, x, n, k) == -4
    assert f(P.h, ar, 0, b, n, None, n, k) == -4
    assert f(P.h, ar, 0, b, n - 1, x, n, k) == -4
    assert f(P.h, ar, 1, b, n, x, n - 1, k) == -4
    assert f(P.h, ar, -1, b, n, x, n, -1) == -4
    assert (X == -7.0).all()
    # nrhs = 0: accepted, nothing is read or written
    assert f(P.h, None, 0, None, n, None, n, 0) == 0
    assert f(P.h, ar, -1, b, n, x, n, 0) == 0
    assert (X == -7.0).all() and (B == 1.0).all()


def test_the_library_has_the_entry_point():
    import cholesky_amd as ca
    L = ca.load()
    assert hasattr(L, "cholamd_plan_solve_det_host_nrhs")
