"""Half solves, the factor's diagonal and log det A on the device (cholamd_solve_half*, cholamd_factor_diag*, cholamd_factor_logdet*).

M = P^T L P in original dof order, M M^T = A.  FORWARD: y = M^-1 b, BACKWARD: x = M^-T z.  References are formed on the host from a factor that
is not the code under test: the CPU oracle's L and the reference project's golden L / x on the four fixtures, the dense fp64 Cholesky factor of
P A P^T on the general inputs of spd_inputs.

Tolerances.  General inputs: spd_inputs' derived bounds -- tol_forward(u) = C_FE (k + 1) u kappa for both halves (FORWARD as max|y - y_ref| /
max|y_ref|: y = L^-1 P b is invariant under a symmetric diagonal scaling of A with b scaled along; BACKWARD as SPD.forward_error), tol_factor(u)
for the diagonal per sqrt(A_ii), and for the logdet C_L (k + 1) u kappa n: to first order log det(A + dA) - log det A = tr(A^-1 dA), and with the
equilibrated backward error |dA_eq| <= gamma_(k+1) entrywise (spd_inputs' docstring) |tr(A_eq^-1 dA_eq)| <= n ||A_eq^-1|| max|dA_eq| <= n kappa
(k + 1) u.  u = 2^-53 for the fp64 factor, 2^-24 for the fp32 one.  Fixtures: the fixture gates (x and y to 1e-10 relative against the oracle,
the diagonal to 1e-12 against golden L for the fp64 factor; one unrefined fp32-factor solve to 1e-3 as test_gpu_poison and test_gpu_mixed hold
it), and the same logdet bound with k, kappa computed here from the golden P A P^T and L.

fp32 factor: every input of spd_inputs is kept (none is excluded)."""
import math
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg as sl

pytestmark = pytest.mark.gpu

import spd_inputs as si  # noqa: E402
from conftest import CASES, ROOT, case_paths  # noqa: E402
from guarded import Guarded  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from spd_inputs import C_L, U32, U64  # noqa: E402

W = 32
NRHS = [1, 3, 16, W - 1, W, W + 1, 2 * W + 5]   # the list of tests/test_gpu_solve_nrhs.py
FWD, BWD = 0, 1
PRECISIONS = [False, True]
PIDS = ["fp64", "fp32"]
EXCLUDED_F32 = []            # inputs the fp32 factor cannot take: none
BIN = os.path.join(ROOT, "cholesky_amd", "bin", "cholamd_mmat")


@pytest.fixture(scope="module")
def ca():
    import cholesky_amd
    orc.use_own_kernels()
    return cholesky_amd


@pytest.fixture(scope="module")
def spd(tmp_path_factory):
    return lambda name: si.cached(tmp_path_factory, name)


def colmajor(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).T)).cuda().T


def nan_block(n, k):
    import torch
    return torch.full((k, n), float("nan"), dtype=torch.float64, device="cuda").T


def factored(ca, plan, f32):
    dev = ca.Device(plan, 0)
    a = dev.new_arena_f32() if f32 else dev.new_arena()
    (dev.fill_f32 if f32 else dev.fill)(a)
    (dev.factor_f32 if f32 else dev.factor)(a)
    dev.sync()
    assert dev.info() == (0, 0)
    return dev, a


def half_ref(L, perm, V, which):
    """M^-1 V (FWD) or M^-T V (BWD), M = P^T L P, columns of V in original order."""
    V = np.asarray(V, dtype=np.float64)
    R = sl.solve_triangular(L, V[perm], lower=True) if which == FWD else sl.solve_triangular(L.T, V[perm], lower=False)
    out = np.empty_like(R)
    out[perm] = R
    return out


def half(dev, arena, v, which):
    import torch
    d_b = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).cuda()
    d_x = torch.full_like(d_b, float("nan"))
    dev.solve_half(arena, d_b, d_x, which)
    dev.sync()
    return d_x.cpu().numpy()


def half_block(dev, arena, V, which):
    B = colmajor(V)
    X = nan_block(V.shape[0], V.shape[1])
    dev.solve_half_nrhs(arena, B, X, which)
    dev.sync()
    return X.cpu().numpy()


def rel_cols(x, ref):
    return np.abs(x - ref).max(axis=0) / np.maximum(np.abs(ref).max(axis=0), 1e-300)


# ------------------------------------------------------------------------------------------------
# the fixtures: oracle, golden, and the terms of the derived bounds
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx(ca, golden):
    cache = {}

    def get(case):
        if case not in cache:
            m, o, c, bf = case_paths(case)
            plan = ca.Plan(m, o, c)
            O = orc.Oracle(m, o, c)
            O.factor()
            assert O.info == 0
            g = golden(case)
            n = plan.n
            perm = np.asarray(O.perm)
            assert np.array_equal(perm, plan.perm)
            Lo = np.tril(O.dense())
            PAP = g["pmat"] + np.tril(g["pmat"], -1).T
            s = np.sqrt(np.diag(PAP))
            ev = np.linalg.eigvalsh(PAP / s[:, None] / s[None, :])
            rng = np.random.default_rng(7)
            V = np.empty((n, max(NRHS)))
            V[:, 0] = ca.plan.read_vector(bf, n)
            V[:, 1:] = rng.standard_normal((n, max(NRHS) - 1))
            cache[case] = dict(plan=plan, Lo=Lo, Lg=g["L"], perm=perm, g=g, V=V, kappa=float(ev[-1] / ev[0]), k=int((g["L"] != 0).sum(axis=1).max()),
                               sp=s, dev={})
        return cache[case]

    return get


def fx_dev(ca, r, f32):
    if f32 not in r["dev"]:
        r["dev"][f32] = factored(ca, r["plan"], f32)
    return r["dev"][f32]


_SPD_DEV = {}


def spd_dev(ca, S, name, f32):
    if (name, f32) not in _SPD_DEV:
        _SPD_DEV[name, f32] = factored(ca, S.plan, f32)
    return _SPD_DEV[name, f32]


def spd_block(S):
    rng = np.random.default_rng(7)
    V = S.s[:, None] * rng.standard_normal((S.n, max(NRHS)))
    V[:, 0] = S.rhs
    return V


def logdet_tol(k, kappa, n, u):
    return C_L * (k + 1) * u * kappa * n


# ------------------------------------------------------------------------------------------------
# 1. half solves against the reference factor
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("case", list(CASES))
def test_half_solves_on_fixtures_match_the_oracle(case, f32, ca, fx):
    r = fx(case)
    dev, arena = fx_dev(ca, r, f32)
    tol = 1e-3 if f32 else 1e-10
    V = r["V"]
    for which in (FWD, BWD):
        ref = half_ref(r["Lo"], r["perm"], V, which)
        x = half(dev, arena, V[:, 0], which)
        e = rel_cols(x[:, None], ref[:, :1]).max()
        print(f"{case} {PIDS[f32]} which={which} single: {e:.3e} (tol {tol:.1e})")
        assert e <= tol
        for k in NRHS:
            X = half_block(dev, arena, V[:, :k], which)
            e = rel_cols(X, ref[:, :k]).max()
            print(f"{case} {PIDS[f32]} which={which} nrhs={k}: {e:.3e} (tol {tol:.1e})")
            assert e <= tol, (which, k)


@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("name", si.NAMES)
def test_half_solves_on_general_inputs_match_the_dense_factor(name, f32, ca, spd):
    assert not (f32 and name in EXCLUDED_F32)
    S = spd(name)
    dev, arena = spd_dev(ca, S, name, f32)
    tol = S.tol_forward(U32 if f32 else U64)
    B = spd_block(S)
    Yref = half_ref(S.Ld, S.perm, B, FWD)          # FORWARD of right-hand sides that scale like b
    Xref = half_ref(S.Ld, S.perm, Yref, BWD)       # BACKWARD of their whitened images: solutions of A x = b

    def fwd_err(Y, k):
        return rel_cols(Y, Yref[:, :k]).max()

    def bwd_err(X, k):
        return max(S.forward_error(X[:, j], Xref[:, j]) for j in range(k))

    e = fwd_err(half(dev, arena, B[:, 0], FWD)[:, None], 1)
    print(f"{name} {PIDS[f32]} FORWARD single: {e:.3e} (tol {tol:.3e})")
    assert e <= tol
    e = bwd_err(half(dev, arena, Yref[:, 0], BWD)[:, None], 1)
    print(f"{name} {PIDS[f32]} BACKWARD single: {e:.3e} (tol {tol:.3e})")
    assert e <= tol
    for k in NRHS:
        e = fwd_err(half_block(dev, arena, B[:, :k], FWD), k)
        print(f"{name} {PIDS[f32]} FORWARD nrhs={k}: {e:.3e} (tol {tol:.3e})")
        assert e <= tol, k
        e = bwd_err(half_block(dev, arena, Yref[:, :k], BWD), k)
        print(f"{name} {PIDS[f32]} BACKWARD nrhs={k}: {e:.3e} (tol {tol:.3e})")
        assert e <= tol, k


# ------------------------------------------------------------------------------------------------
# 2. composition, 3. quadratic form and square root
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("case", list(CASES))
def test_backward_of_forward_is_the_solve(case, f32, ca, fx):
    import torch
    r = fx(case)
    dev, arena = fx_dev(ca, r, f32)
    n, V, gx = r["plan"].n, r["V"], r["g"]["x"]
    k = max(NRHS)
    B = colmajor(V)
    Xs = torch.empty(k, n, dtype=torch.float64, device="cuda").T
    for j in range(k):
        (dev.solve_f32 if f32 else dev.solve)(arena, B[:, j], Xs[:, j])
    dev.sync()
    xs = Xs.cpu().numpy()
    for kk in NRHS:
        Y, X = nan_block(n, kk), nan_block(n, kk)
        dev.solve_half_nrhs(arena, B[:, :kk], Y, FWD)
        dev.solve_half_nrhs(arena, Y, X, BWD)
        dev.sync()
        x = X.cpu().numpy()
        e = rel_cols(x, xs[:, :kk]).max()
        print(f"{case} {PIDS[f32]} BACKWARD(FORWARD(B)) vs solve, nrhs={kk}: {e:.3e}")
        assert e <= 1e-12, kk
        if not f32:
            assert np.abs(x[:, 0] - gx).max() <= 1e-10 * max(1.0, np.abs(gx).max())
    # single vectors, then both forms in place
    y = half(dev, arena, V[:, 0], FWD)
    x = half(dev, arena, y, BWD)
    assert rel_cols(x[:, None], xs[:, :1]).max() <= 1e-12
    t = torch.from_numpy(V[:, 0].copy()).cuda()
    dev.solve_half(arena, t, t, FWD)
    dev.solve_half(arena, t, t, BWD)
    Bp = colmajor(V[:, :W + 1])
    dev.solve_half_nrhs(arena, Bp, Bp, FWD)
    dev.solve_half_nrhs(arena, Bp, Bp, BWD)
    dev.sync()
    assert rel_cols(t.cpu().numpy()[:, None], xs[:, :1]).max() <= 1e-12
    assert rel_cols(Bp.cpu().numpy(), xs[:, :W + 1]).max() <= 1e-12
    if not f32:
        assert np.abs(t.cpu().numpy() - gx).max() <= 1e-10 * max(1.0, np.abs(gx).max())


@pytest.mark.parametrize("case", list(CASES))
def test_quadratic_form_and_square_root(case, ca, fx):
    """||FORWARD(b)||^2 = b^T A^-1 b against b^T x_golden.  Both sides carry the fixture gate of 1e-10 relative in the max norm: the golden x
    changes b^T x by at most ||b||_1 1e-10 max|x|, an error dy in y changes ||y||^2 by at most 2 ||y||_1 max|dy| <= 2 ||y||_1 1e-10 max|y|.
    And A BACKWARD(FORWARD(e)) = e at the fixtures' residual gate."""
    import torch
    r = fx(case)
    dev, arena = fx_dev(ca, r, False)
    b, gx = r["V"][:, 0], r["g"]["x"]        # the fixture's right-hand side file; golden x solves it
    y = half(dev, arena, b, FWD)
    q, qref = float(y @ y), float(b @ gx)
    tol = 1e-10 * (np.abs(b).sum() * np.abs(gx).max() + 2.0 * np.abs(y).sum() * np.abs(y).max())
    print(f"{case}: ||y||^2 = {q!r}, b^T x_golden = {qref!r}, diff {abs(q - qref):.3e} (tol {tol:.3e})")
    assert abs(q - qref) <= tol
    e = torch.from_numpy(r["V"][:, 1].copy()).cuda()
    x = torch.full_like(e, float("nan"))
    dev.solve_half(arena, e, x, FWD)
    dev.solve_half(arena, x, x, BWD)
    rel = dev.residual(e, x)
    print(f"{case}: residual of BACKWARD(FORWARD(e)) = {rel:.3e}")
    assert rel <= 1e-10


# ------------------------------------------------------------------------------------------------
# 4. logdet, 5. factor_diag
# ------------------------------------------------------------------------------------------------
def check_logdet_and_diag(dev, arena, n, perm, Lref, sp, k, kappa, u, tag, diag_tol):
    ld1 = dev.logdet(arena)
    ld2 = dev.logdet(arena)
    ref = 2.0 * math.fsum(np.log(np.diag(Lref)))
    tol = logdet_tol(k, kappa, n, u)
    print(f"{tag}: logdet = {ld1!r}, ref = {ref!r}, diff {abs(ld1 - ref):.3e} (tol {tol:.3e})")
    assert np.float64(ld1).view(np.uint64) == np.float64(ld2).view(np.uint64)       # deterministic: the same bits
    assert abs(ld1 - ref) <= tol
    d = dev.factor_diag(arena)
    dev.sync()
    d = d.cpu().numpy()
    assert np.isfinite(d).all() and (d > 0).all()
    host = 2.0 * math.fsum(np.log(d))
    stol = n * 2.0 ** -52 * np.abs(np.log(d)).max()
    print(f"{tag}: 2 fsum(log diag) - logdet = {abs(host - ld1):.3e} (tol {stol:.3e})")
    assert abs(host - ld1) <= stol
    dref = np.empty(n)
    dref[perm] = np.diag(Lref)
    s = np.empty(n)
    s[perm] = sp
    e = float((np.abs(d - dref) / s).max())
    print(f"{tag}: diag error / sqrt(A_ii) = {e:.3e} (tol {diag_tol:.3e})")
    assert e <= diag_tol
    return d


@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("case", list(CASES))
def test_logdet_and_diag_on_fixtures(case, f32, ca, fx):
    r = fx(case)
    dev, arena = fx_dev(ca, r, f32)
    n, u = r["plan"].n, U32 if f32 else U64
    d = check_logdet_and_diag(dev, arena, n, r["perm"], r["Lg"], r["sp"], r["k"], r["kappa"], u, f"{case} {PIDS[f32]}",
                              C_L * (r["k"] + 1) * u * r["kappa"])
    if not f32:   # the fixtures' own gate against the reference project's L
        dref = np.empty(n)
        dref[r["perm"]] = np.diag(r["Lg"])
        assert np.abs(d - dref).max() <= 1e-12


@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("name", si.NAMES)
def test_logdet_and_diag_on_general_inputs(name, f32, ca, spd):
    assert not (f32 and name in EXCLUDED_F32)
    S = spd(name)
    dev, arena = spd_dev(ca, S, name, f32)
    u = U32 if f32 else U64
    check_logdet_and_diag(dev, arena, S.n, S.perm, S.Ld, S.sp, S.k, S.kappa, u, f"{name} {PIDS[f32]}", S.tol_factor(u))


# ------------------------------------------------------------------------------------------------
# 6. refusals
# ------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_untouched(ca, fx):
    import ctypes as C
    import torch
    r = fx("lapl_400x400")
    n = r["plan"].n
    for f32 in PRECISIONS:
        dev, arena = fx_dev(ca, r, f32)
        L, h, p = dev.L, dev.h, dev.ptr
        one = L.cholamd_solve_half_f32 if f32 else L.cholamd_solve_half
        blk = L.cholamd_solve_half_nrhs_f32 if f32 else L.cholamd_solve_half_nrhs
        b = torch.from_numpy(r["V"][:, 0].copy()).cuda()
        B = colmajor(r["V"][:, :4])
        x = torch.full_like(b, float("nan"))
        X = nan_block(n, 4)
        msg = lambda: ca.load().cholamd_last_error().decode()  # noqa: E731
        assert one(h, p(arena), p(b), p(x), 2, None) == -4 and "which" in msg()
        assert one(h, p(arena), p(b), p(x), -1, None) == -4
        assert blk(h, p(arena), p(B), n, p(X), n, 4, 2, None) == -4 and "which" in msg()
        assert blk(h, p(arena), p(B), n, p(X), n, -1, FWD, None) == -4 and "nrhs" in msg()
        assert blk(h, p(arena), p(B), n - 1, p(X), n, 4, FWD, None) == -4 and "ldb" in msg()
        assert blk(h, p(arena), p(B), n, p(X), n - 1, 4, BWD, None) == -4 and "ldx" in msg()
        assert blk(h, p(arena), None, n, p(X), n, 4, FWD, None) == -4 and "NULL" in msg()
        assert blk(h, None, p(B), n, p(X), n, 4, FWD, None) == -4 and "NULL" in msg()
        assert blk(h, p(arena), p(B), n, None, n, 4, FWD, None) == -4
        assert one(h, p(arena), None, p(x), FWD, None) == -4 and "NULL" in msg()
        assert one(h, None, p(b), p(x), FWD, None) == -4
        assert one(h, p(arena), p(b), None, BWD, None) == -4
        assert blk(h, p(arena), p(B), n, p(X), n, 0, FWD, None) == 0
        assert blk(h, p(arena), None, n, None, n, 0, BWD, None) == 0
        dev.solve_half_nrhs(arena, B[:, :0], X[:, :0], FWD)
        with pytest.raises(ca.CholamdError, match="which"):
            dev.solve_half(arena, b, x, 2)
        dev.sync()
        assert torch.isnan(x).all() and torch.isnan(X).all()
        out = C.c_double(1.0)
        fl = L.cholamd_factor_logdet_f32 if f32 else L.cholamd_factor_logdet
        fd = L.cholamd_factor_diag_f32 if f32 else L.cholamd_factor_diag
        assert fl(h, None, C.byref(out), None) == -4 and math.isnan(out.value)
        assert fl(h, p(arena), None, None) == -4
        assert fd(h, p(arena), None, None) == -4 and fd(h, None, p(x), None) == -4
        assert torch.isnan(x).all()
        with pytest.raises(ValueError):
            dev.factor_diag(arena, out=torch.empty(n + 1, dtype=torch.float64, device="cuda"))


@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
def test_logdet_of_a_nan_arena_names_separator_and_column(f32, ca, fx):
    import ctypes as C
    import torch
    r = fx("lapl_400x400")
    plan = r["plan"]
    dev, _ = fx_dev(ca, r, f32)
    bad = torch.full((plan.arena_doubles,), float("nan"), dtype=torch.float32 if f32 else torch.float64, device="cuda")
    out = C.c_double(1.0)
    fn = dev.L.cholamd_factor_logdet_f32 if f32 else dev.L.cholamd_factor_logdet
    assert fn(dev.h, dev.ptr(bad), C.byref(out), None) == -4
    assert math.isnan(out.value)
    first = int(np.nonzero((plan.sep_offsets == 0) & (plan.sep_sizes > 0))[0][0]) + 1     # the separator at permuted position 0: the first bad entry
    msg = ca.load().cholamd_last_error().decode()
    assert f"column 1 of separator {first} " in msg and f"{plan.n} of the factor's diagonal entries" in msg, msg
    with pytest.raises(ca.CholamdError, match="separator"):
        dev.logdet(bad)


def _diag_index(P, host, k):
    """Arena index of the diagonal entry of permuted position k (located through arena_to_dense)."""
    blocks = P.blocks
    lbl = int(np.nonzero((P.sep_offsets <= k) & (k < P.sep_offsets + P.sep_sizes))[0][0]) + 1
    b = blocks[(blocks[:, 0] == lbl) & (blocks[:, 1] == lbl)][0]
    j = k - int(P.sep_offsets[lbl - 1])
    idx = int(b[7]) + j + j * int(b[6])
    probe = np.zeros_like(host)
    probe[idx] = 1.0
    D = P.arena_to_dense(probe)
    assert D[k, k] == 1.0 and np.count_nonzero(D) == 1
    return idx


@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
def test_logdet_after_a_failed_factorisation_is_refused(f32, ca, spd):
    """The construction of test_pivot_failure_anywhere_reports_its_column (g12_full, a pivot in the middle of a leaf's second tile): A'_kk = A_kk -
    1.5 L_kk^2 makes pivot k the first that fails; info > 0, and the arena is no factor."""
    import torch
    S = spd("g12_full")
    P = S.plan
    lv = P.levels
    lbl = next(lb for lb in range(1, P.nsep + 1) if S.level_of(lb) == lv - 1 and P.sep_sizes[lb - 1] >= 48)
    k = int(P.sep_offsets[lbl - 1]) + 16
    host = P.fill_host()
    host[_diag_index(P, host, k)] = S.PAP[k, k] - 1.5 * S.Ld[k, k] ** 2
    dev = ca.Device(P, 0)
    bad = torch.from_numpy(host.astype(np.float32) if f32 else host).cuda()
    (dev.factor_f32 if f32 else dev.factor)(bad)
    dev.sync()
    off = int(P.sep_offsets[lbl - 1])
    assert dev.info() == (k - off + 1, lbl)
    with pytest.raises(ca.CholamdError, match="code -4") as ei:
        dev.logdet(bad)
    print(f"{PIDS[f32]}: {ei.value}")
    assert "separator" in str(ei.value)


# ------------------------------------------------------------------------------------------------
# 7. set_values interplay
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
def test_logdet_follows_set_values(f32, ca, spd):
    """alpha = 4: L scales by exactly 2, the logdet moves by n log 4 (to the logdet bound: the two sums round on their own)."""
    S = spd("g16_subset")
    dev, arena = factored(ca, S.plan, f32)
    ld0 = dev.logdet(arena)
    vals = np.ascontiguousarray(S.val[np.lexsort((S.row, S.col))])
    dev.set_values(4.0 * vals)
    (dev.fill_f32 if f32 else dev.fill)(arena)
    (dev.factor_f32 if f32 else dev.factor)(arena)
    dev.sync()
    assert dev.info() == (0, 0)
    ld1 = dev.logdet(arena)
    tol = logdet_tol(S.k, S.kappa, S.n, U32 if f32 else U64)
    print(f"{PIDS[f32]}: logdet moved by {ld1 - ld0!r}, n log 4 = {S.n * math.log(4.0)!r}, diff {abs(ld1 - ld0 - S.n * math.log(4.0)):.3e} (tol {tol:.3e})")
    assert abs(ld1 - ld0 - S.n * math.log(4.0)) <= tol


# ------------------------------------------------------------------------------------------------
# 8. poison / guards
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
def test_poisoned_scratch_and_guarded_buffers(f32, ca, spd, monkeypatch):
    import torch
    S = spd("g18_full")
    n, ld, k = S.n, S.n + 3, W + 5
    V = spd_block(S)[:, :k]
    monkeypatch.delenv("CHOLAMD_POISON", raising=False)
    plain = {}
    dev, arena = factored(ca, S.plan, f32)
    for which in (FWD, BWD):
        plain[which] = half_block(dev, arena, V, which)
        plain[which, 1] = half(dev, arena, V[:, 0], which)
    dplain = dev.factor_diag(arena).cpu().numpy()
    ldplain = dev.logdet(arena)
    del dev, arena
    monkeypatch.setenv("CHOLAMD_POISON", "1")
    for v in ("CHOLAMD_SOLVE_NO_BAND", "CHOLAMD_SOLVE_NO_INV256", "CHOLAMD_SOLVE_REFERENCE_SHAPE"):
        monkeypatch.delenv(v, raising=False)
    dev = ca.Device(S.plan, 0)
    a = Guarded(S.plan.arena_doubles, dtype=torch.float32 if f32 else torch.float64)
    (dev.fill_f32 if f32 else dev.fill)(a.t)
    (dev.factor_f32 if f32 else dev.factor)(a.t)
    dev.sync()
    assert dev.info() == (0, 0)
    asnap = a.snapshot()
    for which in (FWD, BWD):
        b, x = Guarded(n, values=V[:, 0]), Guarded(n)
        snap = b.snapshot()
        dev.solve_half(a.t, b.t, x.t, which)
        dev.sync()
        b.assert_unchanged(snap, "b")
        x.assert_guards("x")
        assert rel_cols(x.numpy()[:, None], plain[which, 1][:, None]).max() <= 1e-12
        B, X = Guarded(n, k, ld, values=V), Guarded(n, k, ld)
        snap = B.snapshot()
        dev.solve_half_nrhs(a.t, B.t, X.t, which)
        dev.sync()
        B.assert_unchanged(snap, "B")
        X.assert_guards("X")                  # guards and the padding rows n .. ld - 1
        assert rel_cols(X.numpy(), plain[which]).max() <= 1e-12
        dev.solve_half_nrhs(a.t, B.t, B.t, which)
        dev.sync()
        B.assert_guards("B in place")
        assert rel_cols(B.numpy(), plain[which]).max() <= 1e-12
    dg = Guarded(n)
    dev.factor_diag(a.t, out=dg.t)
    dev.sync()
    dg.assert_guards("diag")
    assert (np.abs(dg.numpy() - dplain) <= 1e-12 * np.abs(dplain)).all()
    assert abs(dev.logdet(a.t) - ldplain) <= 2.0 * n * 1e-12        # every L_ii within 1e-12 relative: every log within 1e-12
    a.assert_unchanged(asnap, "arena")


# ------------------------------------------------------------------------------------------------
# 9. gathered factor
# ------------------------------------------------------------------------------------------------
def test_gathered_factor_on_rank_zero(ca, fx):
    import ctypes as C
    from cholesky_amd import _lib
    from cholesky_amd.device import factor_multi
    r = fx("lapl_3375x3375")
    plan, n = r["plan"], r["plan"].n
    dev1, a1 = fx_dev(ca, r, False)
    ld_single = dev1.logdet(a1)
    y_single = half(dev1, a1, r["V"][:, 0], FWD)
    world = 2
    devs, arenas = [], []
    for g in range(world):
        dev = ca.Device(plan, 0)
        dev.set_partition(g, world)
        a = dev.new_arena()
        dev.fill(a)
        devs.append(dev)
        arenas.append(a)
    factor_multi(devs, arenas, local=True)
    for dev in devs:
        assert dev.info() == (0, 0)
    hd = (C.c_void_p * world)(*[d.h for d in devs])
    ha = (C.c_void_p * world)(*[C.c_void_p(a.data_ptr()) for a in arenas])
    _lib.check(devs[0].L.cholamd_gather_factor(hd, ha, world, None), "cholamd_gather_factor")
    devs[0].sync()
    ld = devs[0].logdet(arenas[0])
    ref = 2.0 * math.fsum(np.log(np.diag(r["Lg"])))
    tol = logdet_tol(r["k"], r["kappa"], n, U64)
    print(f"gathered: logdet {ld!r}, single GPU {ld_single!r}, ref {ref!r} (tol {tol:.3e})")
    assert abs(ld - ref) <= tol and abs(ld - ld_single) <= tol
    y = half(devs[0], arenas[0], r["V"][:, 0], FWD)
    yref = half_ref(r["Lo"], r["perm"], r["V"][:, :1], FWD)
    assert rel_cols(y[:, None], yref).max() <= 1e-10
    assert rel_cols(y[:, None], y_single[:, None]).max() <= 1e-10


# ------------------------------------------------------------------------------------------------
# 10. the command line
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixed", [False, True], ids=PIDS)
def test_cli_logdet_line(mixed, tmp_path, fx, golden):
    case = "lapl_3375x3375"
    r = fx(case)
    m, o, c, b = case_paths(case)
    outs = []
    for flag in (False, True):
        sol = tmp_path / f"x{int(flag)}.txt"
        args = [BIN, "-i", m, "-s", o, "-c", c, "-b", b, "-o", str(sol), "--full-precision"] + (["--precision", "mixed"] if mixed else []) + (["--logdet"] if flag else [])
        p = subprocess.run(args, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        outs.append((p.stdout.replace(str(sol), "SOL"), np.genfromtxt(str(sol))))
    tag = "logdet(fp32 factor): " if mixed else "logdet: "
    lines = [ln for ln in outs[1][0].splitlines() if "logdet" in ln]
    assert len(lines) == 1 and lines[0].startswith(tag), lines
    assert "logdet" not in outs[0][0]
    assert [ln for ln in outs[1][0].splitlines() if "logdet" not in ln] == outs[0][0].splitlines()     # nothing else changes
    val = float(lines[0][len(tag):])
    assert lines[0] == tag + "%.17g" % val
    ref = 2.0 * math.fsum(np.log(np.diag(r["Lg"])))
    tol = logdet_tol(r["k"], r["kappa"], r["plan"].n, U32 if mixed else U64)
    print(f"cli {PIDS[mixed]}: {lines[0]} ref {ref!r} (tol {tol:.3e})")
    assert abs(val - ref) <= tol
    gx = golden(case)["x"]
    for _, x in outs:
        assert np.abs(x - gx).max() <= 1e-10 * max(1.0, np.abs(gx).max())
