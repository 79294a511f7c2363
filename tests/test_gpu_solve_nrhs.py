"""Block solve (cholamd_solve_nrhs / _f32 / cholamd_solve_refine_nrhs): many right-hand sides per pass over the factor, checked column by column
against the single-vector solve, the CPU oracle and the reference's golden x, through every chunk boundary of the 32-column chunks."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import CASES, case_paths
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

W = 32  # right-hand sides per chunk (CHOL_NRHS_W)
NRHS = [1, 3, 16, W - 1, W, W + 1, 2 * W + 5]


@pytest.fixture(scope="module")
def ca():
    import cholesky_amd
    orc.use_own_kernels()
    return cholesky_amd


def colmajor(a):
    """(n, k) numpy -> CUDA float64 tensor of the same shape with stride(0) == 1 (ld = n)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).T)).cuda().T


def rel_err(x, ref):
    return np.abs(x - ref).max(axis=0) / np.maximum(np.abs(ref).max(axis=0), 1e-300)


def single_solves(dev, arena, B, f32=False):
    import torch
    X = torch.empty(B.shape[1], B.shape[0], dtype=torch.float64, device=B.device).T
    for j in range(B.shape[1]):
        (dev.solve_f32 if f32 else dev.solve)(arena, B[:, j], X[:, j])
    dev.sync()
    return X.cpu().numpy()


def residuals(dev, B, X):
    return np.array([dev.residual(B[:, j], X[:, j]) for j in range(B.shape[1])])


def factored(ca, plan, f32=False):
    dev = ca.Device(plan, 0)
    a = dev.new_arena()
    dev.fill(a)
    dev.factor(a)
    a32 = None
    if f32:
        a32 = dev.new_arena_f32()
        dev.fill_f32(a32)
        dev.factor_f32(a32)
    dev.sync()
    assert dev.info() == (0, 0)
    return dev, a, a32


@pytest.fixture(scope="module")
def fixtures(ca):
    out = {}
    rng = np.random.default_rng(7)
    for case in CASES:
        m, o, c, b = case_paths(case)
        plan = ca.Plan(m, o, c)
        dev, arena, _ = factored(ca, plan)
        n = plan.n
        Bh = np.empty((n, max(NRHS)))
        Bh[:, 0] = ca.plan.read_vector(b, n)
        Bh[:, 1:] = rng.standard_normal((n, max(NRHS) - 1))
        B = colmajor(Bh)
        O = orc.Oracle(m, o, c)
        O.factor()
        Xo = np.stack([O.solve(Bh[:, j]) for j in range(Bh.shape[1])], axis=1)
        out[case] = dict(plan=plan, dev=dev, arena=arena, Bh=Bh, B=B, Xs=single_solves(dev, arena, B), Xo=Xo)
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_block_solve_matches_single_solves_oracle_and_golden(case, fixtures, golden):
    import torch
    r = fixtures[case]
    dev, arena, B = r["dev"], r["arena"], r["B"]
    n = r["plan"].n
    for k in NRHS:
        X = torch.full((k, n), float("nan"), dtype=torch.float64, device="cuda").T
        dev.solve_nrhs(arena, B[:, :k], X)
        dev.sync()
        x = X.cpu().numpy()
        assert (rel_err(x, r["Xs"][:, :k]) <= 1e-12).all(), (k, rel_err(x, r["Xs"][:, :k]).max())
        assert (rel_err(x, r["Xo"][:, :k]) <= 1e-10).all(), (k, rel_err(x, r["Xo"][:, :k]).max())
        gx = golden(case)["x"]
        assert np.abs(x[:, 0] - gx).max() <= 1e-10 * max(1.0, np.abs(gx).max())
        assert (residuals(dev, B[:, :k], X) <= 1e-10).all()


def test_leading_dimensions_padding_and_in_place(fixtures):
    import torch
    r = fixtures["lapl_3375x3375"]
    dev, arena, Bh = r["dev"], r["arena"], r["Bh"]
    n, k = r["plan"].n, 2 * W + 5
    Bp = torch.zeros(k, n + 5, dtype=torch.float64, device="cuda")
    Bp[:, :n] = torch.from_numpy(np.ascontiguousarray(Bh[:, :k].T)).cuda()
    B = Bp[:, :n].T
    assert B.stride() == (1, n + 5)
    Xp = torch.full((k, n + 3), float("nan"), dtype=torch.float64, device="cuda")
    X = Xp[:, :n].T
    before = Bp.cpu().numpy().copy()
    dev.solve_nrhs(arena, B, X)
    dev.sync()
    assert np.array_equal(Bp.cpu().numpy(), before)                        # B untouched, padding included
    assert torch.isnan(Xp[:, n:]).all()                                     # X's padding rows never written
    x = X.cpu().numpy()
    assert (rel_err(x, r["Xs"][:, :k]) <= 1e-12).all()
    dev.solve_nrhs(arena, B, B)                                             # in place (X is B)
    dev.sync()
    assert np.array_equal(Bp[:, n:].cpu().numpy(), before[:, n:])
    assert (rel_err(B.cpu().numpy(), r["Xs"][:, :k]) <= 1e-12).all()


GRIDS = [(24, 24, 24, 5, 32), (18, 18, 18, 3, 48), (12, 12, 12, 4, 16)]


@pytest.mark.parametrize("dims", GRIDS)
def test_generated_grids_fp64_fp32_and_refinement(dims, ca, tmp_path):
    import torch
    prob = ca.Problem(*dims)
    plan = prob.plan()
    n, k = plan.n, W + 7
    m, o, c, _ = prob.write(os.path.join(tmp_path, "gen"))
    O = orc.Oracle(m, o, c)
    O.factor()
    rng = np.random.default_rng(11)
    Bh = np.empty((n, k))
    Bh[:, 0] = prob.rhs()
    Bh[:, 1:] = rng.standard_normal((n, k - 1))
    Xo = np.stack([O.solve(Bh[:, j]) for j in range(k)], axis=1)
    B = colmajor(Bh)
    dev, a, a32 = factored(ca, plan, f32=True)
    for arena, f32 in ((a, False), (a32, True)):
        X = torch.empty(k, n, dtype=torch.float64, device="cuda").T
        dev.solve_nrhs(arena, B, X)
        dev.sync()
        x = X.cpu().numpy()
        assert (rel_err(x, single_solves(dev, arena, B, f32)) <= 1e-12).all(), (f32, dims)
        if not f32:
            assert (rel_err(x, Xo) <= 1e-10).all()
            assert (residuals(dev, B, X) <= 1e-10).all()
    X = torch.empty(k, n, dtype=torch.float64, device="cuda").T
    it, rel = dev.solve_refine_nrhs(a32, B, X, max_iter=20, tol=1e-12)
    assert rel.shape == (k,) and (rel <= 1e-12).all() and 0 < it <= 20, (it, rel.max())
    assert np.allclose(rel, residuals(dev, B, X), rtol=1e-6, atol=1e-16)
    assert (rel_err(X.cpu().numpy(), Xo) <= 1e-10).all()


@pytest.mark.parametrize("switch", ["CHOLAMD_SOLVE_NO_INV256", "CHOLAMD_SOLVE_NO_BAND", "solve_reference_shape"])
def test_fallback_switches_give_the_same_x(switch, ca, monkeypatch):
    import torch
    prob = ca.Problem(24, 24, 24, 5, 32)
    plan = prob.plan()
    n, k = plan.n, W + 3
    rng = np.random.default_rng(3)
    B = colmajor(rng.standard_normal((n, k)))
    monkeypatch.delenv("CHOLAMD_SOLVE_NO_INV256", raising=False)
    monkeypatch.delenv("CHOLAMD_SOLVE_NO_BAND", raising=False)
    dev, a, _ = factored(ca, plan)
    X0 = torch.empty(k, n, dtype=torch.float64, device="cuda").T
    dev.solve_nrhs(a, B, X0)
    dev.sync()
    if switch == "solve_reference_shape":
        dev.set_option(switch, 1)
    else:
        monkeypatch.setenv(switch, "1")
        dev, a, _ = factored(ca, plan)
    X1 = torch.empty(k, n, dtype=torch.float64, device="cuda").T
    dev.solve_nrhs(a, B, X1)
    dev.sync()
    assert (rel_err(X1.cpu().numpy(), X0.cpu().numpy()) <= 1e-12).all()


def test_errors_and_empty_calls(fixtures, ca):
    import torch
    r = fixtures["lapl_400x400"]
    dev, arena, B = r["dev"], r["arena"], r["B"]
    n = r["plan"].n
    X = torch.full((4, n), 5.0, dtype=torch.float64, device="cuda").T
    L, h, p = dev.L, dev.h, dev.ptr
    for args, what in (((B, n, X, n, -1), "nrhs"), ((B, n - 1, X, n, 4), "ldb"), ((B, n, X, n - 1, 4), "ldx")):
        Bt, ldb, Xt, ldx, k = args
        for fn, ar in ((L.cholamd_solve_nrhs, arena), (L.cholamd_solve_nrhs_f32, arena)):
            with pytest.raises(ca.CholamdError, match=what):
                ca._lib.check(fn(h, p(ar), p(Bt), ldb, p(Xt), ldx, k, None), "cholamd_solve_nrhs")
        it = C.c_int(0)
        with pytest.raises(ca.CholamdError, match=what):
            ca._lib.check(L.cholamd_solve_refine_nrhs(h, p(arena), p(Bt), ldb, p(Xt), ldx, k, 5, 1e-12, C.byref(it), None, None), "refine")
    with pytest.raises(ca.CholamdError, match="NULL"):
        ca._lib.check(L.cholamd_solve_nrhs(h, p(arena), None, n, p(X), n, 4, None), "cholamd_solve_nrhs")
    assert L.cholamd_solve_nrhs(h, p(arena), p(B), n, p(X), n, 0, None) == 0
    assert L.cholamd_solve_nrhs(h, p(arena), None, n, None, n, 0, None) == 0
    dev.solve_nrhs(arena, B[:, :0], X[:, :0])
    dev.sync()
    assert (X.cpu().numpy() == 5.0).all()
    for bad in (torch.empty(n, 4, dtype=torch.float64, device="cuda"),      # row-major
                torch.empty(4, n, dtype=torch.float32, device="cuda").T,     # fp32
                torch.empty(4, n, dtype=torch.float64).T,                    # host memory
                torch.empty(n, dtype=torch.float64, device="cuda"),          # 1-D
                torch.zeros(n, dtype=torch.float64, device="cuda").unsqueeze(1).expand(n, 4),            # one column repeated: stride (1, 0)
                torch.zeros(4 * n, dtype=torch.float64, device="cuda").as_strided((n, 4), (1, n - 1))):  # overlapping columns
        with pytest.raises(ValueError):
            dev.solve_nrhs(arena, bad, X)
        with pytest.raises(ValueError):
            dev.solve_nrhs(arena, B[:, :4], bad)
        with pytest.raises(ValueError):
            dev.solve_refine_nrhs(arena, B[:, :4], bad)
    assert (X.cpu().numpy() == 5.0).all()


def test_sixty_cubed_fp64_32_right_hand_sides(ca):
    import torch
    prob = ca.Problem(60, 60, 60, 8, 64)
    plan = prob.plan()
    n, k = plan.n, 32
    dev, a, _ = factored(ca, plan)
    rng = np.random.default_rng(5)
    Bh = rng.standard_normal((n, k))
    Bh[:, 0] = prob.rhs()
    B = colmajor(Bh)
    X = torch.empty(k, n, dtype=torch.float64, device="cuda").T
    dev.solve_nrhs(a, B, X)
    dev.sync()
    assert (rel_err(X.cpu().numpy(), single_solves(dev, a, B)) <= 1e-12).all()
    assert (residuals(dev, B, X) <= 1e-10).all()


def test_refinement_in_place_and_after_a_nan(ca, tmp_path):
    """X is B: every chunk's right-hand sides are kept apart before its first solve, so the residuals are those of B (a chunk of 32 columns and one of
    5, which goes column by column).  A NaN column fails the call, and the columns of the chunks after it report NaN."""
    import torch
    prob = ca.Problem(12, 12, 12, 4, 16)
    plan = prob.plan()
    n, k = plan.n, W + 5
    m, o, c, _ = prob.write(os.path.join(tmp_path, "gen"))
    O = orc.Oracle(m, o, c)
    O.factor()
    rng = np.random.default_rng(13)
    Bh = rng.standard_normal((n, k))
    Xo = np.stack([O.solve(Bh[:, j]) for j in range(k)], axis=1)
    dev, _, a32 = factored(ca, plan, f32=True)
    X = colmajor(Bh)
    it2, rel2 = dev.solve_refine_nrhs(a32, X, X)
    assert (rel2 <= 1e-12).all() and 0 < it2 <= 20, (it2, rel2.max())
    assert (rel_err(X.cpu().numpy(), Xo) <= 1e-10).all()
    assert (residuals(dev, colmajor(Bh), X) <= 1e-12).all()
    Bn = Bh.copy()
    Bn[3, 2] = np.nan
    B = colmajor(Bn)
    Xn = torch.empty(k, n, dtype=torch.float64, device="cuda").T
    relres = np.zeros(k)
    iters = C.c_int(-1)
    rc = dev.L.cholamd_solve_refine_nrhs(dev.h, dev.ptr(a32), dev.ptr(B), n, dev.ptr(Xn), n, k, 20, 1e-12, C.byref(iters), relres.ctypes.data, None)
    assert rc != 0 and "NaN" in ca.load().cholamd_last_error().decode()
    assert np.isnan(relres[2]) and np.isnan(relres[W:]).all() and 0 <= iters.value <= 20
