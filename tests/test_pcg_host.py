"""cholamd_plan_apply_host (y = A x in the device's fma order) and the numpy restatement of the PCG loop (tests/pcg_ref.py), without a GPU.

The second half is what makes the iteration caps of tests/test_gpu_pcg.py conditions and not measurements: the reference loop, which shares nothing with
the library but the algorithm, meets every cap on every input of the GPU suite."""
import ctypes as C

import numpy as np
import pytest

import pcg_ref as pr
import spd_inputs as si
from test_values_grad_host import _with_explicit_zero

APPLY_INPUTS = ["lapl_9x9", "lapl_25x25", "g7_ragged", "tree_tiny"]
U64 = 2.0 ** -53


def check_apply(plan, A_sparse, x, y):
    """row by row within (nnz_row + 1) u (|A| |x|)_i of the long-double product"""
    A = A_sparse.toarray().astype(np.longdouble)
    want = A @ x.astype(np.longdouble)
    nnz_row = (A != 0).sum(axis=1)
    bound = (nnz_row + 1) * U64 * (np.abs(A) @ np.abs(x).astype(np.longdouble))
    err = np.abs(y.astype(np.longdouble) - want)
    assert (err <= bound).all(), float((err / np.maximum(bound, np.finfo(float).tiny)).max())


@pytest.mark.parametrize("name", APPLY_INPUTS)
def test_apply_host_against_long_double(tmp_path_factory, name):
    S = si.cached(tmp_path_factory, name)
    rng = np.random.default_rng(3)
    x = rng.standard_normal(S.n) / S.s
    y = S.plan.apply_host(x)
    check_apply(S.plan, S.A_sparse, x, y)
    assert np.array_equal(y, S.plan.apply_host(x, values=pr.values(S)))  # the plan's own values as a value array: the same bits
    # another value array on the pattern
    v = pr.values(S) * rng.uniform(0.5, 2.0, S.plan.nz)
    import scipy.sparse as sp
    check_apply(S.plan, sp.csr_matrix(pr.dense_of(S.plan, v)), x, S.plan.apply_host(x, values=v))


def test_apply_host_skips_explicit_zeros(tmp_path):
    """An entry that was an explicit zero when the plan was made is not part of the operator, whatever the value array says there."""
    S, k = _with_explicit_zero(tmp_path)
    rng = np.random.default_rng(4)
    x = rng.standard_normal(S.n)
    check_apply(S.plan, S.A_sparse, x, S.plan.apply_host(x))
    r, c = S.plan.entries()
    v = np.ascontiguousarray(S.A[r, c])  # the file's values in the plan's entry order
    assert v[k] == 0.0 and np.count_nonzero(v) == S.plan.nz - 1
    y0 = S.plan.apply_host(x, values=v)
    assert np.array_equal(y0, S.plan.apply_host(x))
    v[k] = 123.0
    assert np.array_equal(y0, S.plan.apply_host(x, values=v))


def test_apply_host_arguments(tmp_path_factory):
    import cholesky_amd as ca
    S = si.cached(tmp_path_factory, "lapl_9x9")
    plan, L = S.plan, S.plan.L
    x, y = np.ones(plan.n), np.full(plan.n, 7.0)
    for args, word in (((plan.h, None, None, y.ctypes.data), "NULL x"), ((plan.h, None, x.ctypes.data, None), "NULL y"),
                       ((None, None, x.ctypes.data, y.ctypes.data), "NULL plan"), ((plan.h, None, x.ctypes.data, x.ctypes.data), "y is x")):
        assert L.cholamd_plan_apply_host(*[C.c_void_p(a) if isinstance(a, int) else a for a in args]) == -4
        assert word in L.cholamd_last_error().decode()
    assert (y == 7.0).all() and (x == 1.0).all()
    with pytest.raises(ValueError):
        plan.apply_host(x, values=np.ones(plan.nz + 1))
    assert issubclass(ca.CholamdError, RuntimeError)


# ---- the reference loop meets the gates of the GPU suite ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pr.GPU_INPUTS)
def test_reference_scaled(tmp_path_factory, name):
    """A' = 3 A: one step with the fp64 factor (cap 2); the fp32 factor's count is the GPU cap's base; the stationary refinement diverges."""
    import scipy.linalg as sl
    case = pr.scaled(pr.spd(tmp_path_factory, name))
    B = case.rhs(pr.nrhs_of(name))
    for j in range(B.shape[1]):  # every column of the GPU test
        b = B[:, j]
        x, it, rel, st = case.pcg(b)
        assert st == 0 and it <= 2, (j, it, rel, st)
        case.check_converged(x, b, rel)
        x, it32, rel, st = case.pcg(b, f32=True)
        assert st == 0 and it32 <= pr.MAX_ITER - 1, (j, it32, rel)  # (the GPU cap it32 + 1 is one the loop can miss)
        case.check_converged(x, b, rel)
    b = B[:, 0]
    # x += M^-1 (b - A' x) has the iteration matrix -2 I here
    L32, xr = case.L(np.float32), sl.cho_solve((case.L(np.float32), True), b)
    for _ in range(20):
        xr = xr + sl.cho_solve((L32, True), b - case.Ap @ xr)
    assert not pr.relres_ld(case.Ap, xr, b) <= pr.TOL


@pytest.mark.parametrize("m", [1, 3, 8])
@pytest.mark.parametrize("name", pr.GPU_INPUTS)
def test_reference_rank(tmp_path_factory, name, m):
    case, B = pr.rank_inputs(pr.spd(tmp_path_factory, name), name, m)
    for j in range(B.shape[1]):  # every column of the GPU test
        x, it, rel, st = case.pcg(B[:, j])
        assert st == 0 and it <= m + 2, (j, it, rel, st)
        case.check_converged(x, B[:, j], rel)


@pytest.mark.parametrize("name", pr.GPU_INPUTS + [pr.BIG])
def test_reference_drift(tmp_path_factory, name):
    case = pr.drift(pr.spd(tmp_path_factory, name))
    B = case.rhs(pr.drift_nrhs(name))
    bound = case.drift_bound()
    for j in range(B.shape[1]):  # every column of the GPU test
        b = B[:, j]
        x, it, rel, st = case.pcg(b)
        print(f"{name}, column {j}: kp = {case.kp():.2f}, reference {it} steps, bound {bound}")
        assert st == 0 and it <= bound, (j, it, bound, rel, st)
        case.check_converged(x, b, rel)
        x, _, rel, st = case.pcg(b, f32=True)  # the float32 factor of A as the preconditioner
        assert st == 0, (j, rel, st)
        case.check_converged(x, b, rel)
        # the previous solution as the start vector never costs more steps; the solution itself costs none
        xs = case.x_star(b)
        assert case.pcg(b, x0=xs)[1] == 0
        x_prev = pr.pcg(case.A, case.L(), b)[0]
        assert case.pcg(b, x0=x_prev)[1] <= it
    if name in ("lapl_400x400", "tree_over"):  # the five columns of the deterministic and poisoned runs
        B = case.rhs(5, seed=3)
        for j in range(5):
            x, it, rel, st = case.pcg(B[:, j])
            assert st == 0 and it <= bound, (j, it, bound, rel, st)
            case.check_converged(x, B[:, j], rel)


@pytest.mark.parametrize("name", ["lapl_25x25", "tree_over"])
def test_reference_failure_paths(tmp_path_factory, name):
    S = pr.spd(tmp_path_factory, name)
    case, row = pr.indefinite(S)
    b = np.zeros(S.n)
    b[row] = 1.0
    assert case.Ap[row, row] < 0
    x, it, rel, st = case.pcg(b)
    assert st == pr.BREAKDOWN and np.isfinite(x).all()
    case = pr.drift(S)
    b = case.rhs()[:, 0]
    assert case.pcg(b, max_iter=0)[1:] == (0, 1.0, pr.MAXITER)
    assert case.pcg(np.zeros(S.n))[1:] == (0, 0.0, pr.CONVERGED)
    bn = b.copy()
    bn[0] = np.nan
    assert case.pcg(bn)[3] == pr.NAN
