"""Host restatement of the block products with the factor (cholamd_plan_multiply_host_nrhs): the owner lists of cholamd_multiply_half_nrhs walked over a
host arena with the block kernel's own partition of a source (chol_plan.h: chol_muln_wave, chol_muln_elem -- the split of a reduction range over the
waves, the triangle mask and the clamp, the code the kernel includes) -- no device needed.

Inputs: the four fixtures and every synthetic tree of tree_inputs.NAMED + SINGLE.  The arena holds an independent factor -- the dense fp64 Cholesky factor
of P A P^T -- on the stored positions of the lower triangle and NaN everywhere else (the upper triangles of the diagonal blocks, all padding), so a NaN in
Y means the walk let something take part that is not part of the factor.  Z and Y have leading dimensions larger than n; Plan.multiply_host_nrhs checks that
the rows past n of Y are not written.

Gates (multiply_ref and test_gpu_multiply; nothing is measured):
 1. a half product, per column: componentwise (k + 2) u |L| |z| against tril(arena_to_dense(arena)) applied in extended precision, k = the most stored
    entries in a row (FORWARD) or column (BACKWARD), u = 2^-53 -- the inner-product bound, valid for any summation order, hence for the four partial
    tiles of the block form;
 4. the full product against A Z: |y - A z| <= C_BE (k + 1) u |L| |L^T| |z| componentwise, C_BE = 4 (gate 4 of test_gpu_multiply.py), k = the most stored
    entries in a row of L."""
import ctypes as C

import numpy as np
import pytest

import multiply_ref as mr
import spd_inputs as si
import tree_inputs
from conftest import CASES, case_paths
from spd_inputs import C_BE, U64

NAMES = list(CASES) + tree_inputs.NAMED + tree_inputs.SINGLE
NRHS = [1, 17, 32, 33]
_INPUT = {}


@pytest.fixture(autouse=True)
def environment(monkeypatch):
    for v in ("CHOLAMD_COMPACT", "CHOLAMD_SOLVE_NO_BAND"):
        monkeypatch.delenv(v, raising=False)


def load(name, tmp_path_factory):
    """Once per input: the plan, the arena with NaN outside the lower triangles, and the references of ONE block Z of max(NRHS) columns (a call with fewer
    columns takes the first ones): per direction (Yref, |L| |Z|, k) in extended precision, and A Z with gate 4's bound for the full product."""
    if name not in _INPUT:
        import scipy.sparse as sps
        import cholesky_amd as ca
        if name in CASES:
            plan = ca.Plan(*case_paths(name)[:3])
        else:
            spec = tree_inputs.TREES[name]
            plan = si.SPD(str(tmp_path_factory.mktemp(name)), spec, 3000 + spec["seed"], name=name, oracle=False, dense=False).plan
        n, perm = plan.n, plan.perm
        D = plan.arena_to_dense(plan.fill_host())
        PAP = np.tril(D) + np.tril(D, -1).T
        arena = mr.arena_from_lower(plan, np.linalg.cholesky(PAP))
        assert np.isnan(arena).any() or n == 1, "the upper triangles and the padding hold NaN"
        Dl, mask = mr.stored_lower(plan, arena)
        assert np.isfinite(Dl).all()
        Dsp = sps.csr_matrix(Dl)
        Z = np.random.default_rng(40).standard_normal((n, max(NRHS)))
        ref = {}
        for which in (mr.FWD, mr.BWD):
            cols = [mr.product_sparse(Dsp, perm, Z[:, j], which)[:2] for j in range(Z.shape[1])]
            ref[which] = (np.stack([c[0] for c in cols], axis=1), np.stack([c[1] for c in cols], axis=1), mr.longest(mask, which))
        aD = abs(Dsp)
        AZ, bound = np.empty_like(Z), np.empty_like(Z)
        AZ[perm] = sps.csr_matrix(PAP) @ Z[perm]
        bound[perm] = C_BE * (mr.longest(mask, mr.FWD) + 1) * U64 * (aD @ (aD.T @ np.abs(Z[perm])))
        _INPUT[name] = (plan, arena, Z, ref, AZ, bound)
    return _INPUT[name]


@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("name", NAMES)
def test_half_products_match_the_dense_image(name, nrhs, tmp_path_factory):
    plan, arena, Z, ref, _, _ = load(name, tmp_path_factory)
    n = plan.n
    worst = 0.0
    for which in (mr.FWD, mr.BWD):
        Y = plan.multiply_host_nrhs(arena, which, Z[:, :nrhs], ldz=n + 5, ldy=n + 3)
        Yref, absprod, k = ref[which]
        for j in range(nrhs):
            r = mr.gate_ratio(Y[:, j], Yref[:, j], absprod[:, j], k)
            assert r <= 1.0, (name, which, j, r)
            worst = max(worst, r)
    print(f"{name} nrhs={nrhs}: largest error / gate = {worst:.3f}")


@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("name", NAMES)
def test_full_product_matches_a_z(name, nrhs, tmp_path_factory):
    plan, arena, Z, _, AZ, bound = load(name, tmp_path_factory)
    n = plan.n
    Y = plan.multiply_host_nrhs(arena, -1, Z[:, :nrhs], ldz=n + 1, ldy=n + 7)
    assert np.isfinite(Y).all()
    r = float((np.abs(Y - AZ[:, :nrhs]) / bound[:, :nrhs]).max())
    print(f"{name} nrhs={nrhs}: M M^T Z against A Z, error / gate = {r:.3e}")
    assert r <= 1.0
    # the full product is the FORWARD product of the BACKWARD product, bit for bit
    W = plan.multiply_host_nrhs(arena, mr.BWD, Z[:, :nrhs])
    assert np.array_equal(plan.multiply_host_nrhs(arena, mr.FWD, W), Y)


def test_columns_do_not_depend_on_their_chunk(tmp_path_factory):
    """Column j of a 33-column call, alone in a call of its own: the same bits (a chunk's padding columns and its other columns do not reach it)."""
    plan, arena = load("tree_over", tmp_path_factory)[:2]
    Z = np.random.default_rng(60).standard_normal((plan.n, 33))
    for which in (mr.FWD, mr.BWD, -1):
        Y = plan.multiply_host_nrhs(arena, which, Z)
        for j in (0, 31, 32):
            assert np.array_equal(plan.multiply_host_nrhs(arena, which, Z[:, j:j + 1])[:, 0], Y[:, j]), (which, j)


def test_in_place_returns_the_same_bits(tmp_path_factory):
    plan, arena = load("lapl_400x400", tmp_path_factory)[:2]
    n, k, ld = plan.n, 33, plan.n + 2
    Z = np.random.default_rng(61).standard_normal((n, k))
    f = plan.L.cholamd_plan_multiply_host_nrhs
    for which in (mr.FWD, mr.BWD, -1):
        buf = np.full((k, ld), -3.0)
        buf[:, :n] = Z.T
        assert f(plan.h, arena.ctypes.data, which, buf.ctypes.data, ld, buf.ctypes.data, ld, k) == 0
        assert np.array_equal(buf[:, :n].T, plan.multiply_host_nrhs(arena, which, Z)) and (buf[:, n:] == -3.0).all()


def test_bad_arguments_are_refused(tmp_path_factory):
    plan, arena = load("lapl_9x9", tmp_path_factory)[:2]
    n = plan.n
    z, y = np.ones((2, n)), np.full((2, n), -7.0)
    f = plan.L.cholamd_plan_multiply_host_nrhs
    A, Zp, Yp = arena.ctypes.data, z.ctypes.data, y.ctypes.data
    msg = lambda: plan.L.cholamd_last_error().decode()  # noqa: E731
    for which in (2, -2):
        assert f(plan.h, A, which, Zp, n, Yp, n, 2) == -4 and "which" in msg()
    assert f(plan.h, A, 0, Zp, n, Yp, n, -1) == -4 and "nrhs" in msg()
    assert f(plan.h, A, 0, Zp, n - 1, Yp, n, 2) == -4 and "leading" in msg()
    assert f(plan.h, A, 1, Zp, n, Yp, n - 1, 2) == -4
    assert f(plan.h, None, 0, Zp, n, Yp, n, 2) == -4 and "NULL" in msg()
    assert f(plan.h, A, 0, None, n, Yp, n, 2) == -4
    assert f(plan.h, A, -1, Zp, n, None, n, 2) == -4
    assert f(None, A, 0, Zp, n, Yp, n, 2) == -4
    assert f(plan.h, None, 0, None, n, None, n, 0) == 0, "nrhs == 0 returns 0 and touches nothing"
    assert (y == -7.0).all()


def test_device_entry_points_refuse_a_null_device():
    import cholesky_amd as ca
    L = ca.load()
    buf = (C.c_double * 4)()
    p = C.addressof(buf)
    for sfx in ("", "_f32"):
        assert getattr(L, "cholamd_multiply_half_nrhs" + sfx)(None, p, p, 1, p, 1, 1, 0, None) == -4
        assert "NULL device" in L.cholamd_last_error().decode()
        assert getattr(L, "cholamd_multiply_nrhs" + sfx)(None, p, p, 1, p, 1, 1, None) == -4
        assert "NULL device" in L.cholamd_last_error().decode()
