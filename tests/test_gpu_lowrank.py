"""Low-rank updates, downdates and linear constraints on a factored A on the device (cholamd_lowrank_*, cholesky_amd.LowRank).

Inputs, builders of U, the numpy restatement, the dense references and the gates are those of tests/lowrank_ref.py (all gates derived, none measured from
the code under test).  ldu, ldb, ldx = n + 3 in guarded blocks (tests/guarded.py) wherever a block is passed.  Every test prints its largest error / gate
ratio with pytest -s; DESIGN.md section 15 records them."""
import contextlib
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import lowrank_ref as lr  # noqa: E402
import tree_inputs  # noqa: E402
from guarded import Guarded  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from guarded import G as GUARD  # noqa: E402
from spd_inputs import C_L, U64  # noqa: E402

ERR_ARG = -4
INPUTS = ["lapl_9x9", "lapl_25x25", "lapl_400x400", "lapl_3375x3375", "lapl_3375_scaled", "g7_ragged", "tree_over"]
MODE_IDS = ["update", "downdate", "constraint"]
POISON_INPUTS = ["lapl_400x400", "tree_over"]
SIZES = {"lapl_9x9": 9, "lapl_25x25": 25, "lapl_400x400": 400, "lapl_3375x3375": 3375, "lapl_3375_scaled": 3375, "g7_ragged": 105, "tree_over": 1063}


def logdet_tol(S):
    """Device.logdet's gate (tests/test_gpu_factor_query.py): C_L (k + 1) u kappa n."""
    return C_L * (S.k + 1) * U64 * S.kappa * S.n


@pytest.fixture(scope="module")
def ca():
    import cholesky_amd
    orc.use_own_kernels()
    return cholesky_amd


@pytest.fixture(scope="module")
def spd(tmp_path_factory):
    return lambda name: tree_inputs.cached(tmp_path_factory, name)


def factored(ca, plan):
    dev = ca.Device(plan, 0)
    a = dev.new_arena()
    dev.fill(a)
    dev.factor(a)
    dev.sync()
    assert dev.info() == (0, 0)
    return dev, a


_DEV = {}


def device_of(ca, name, S):
    """(dev, arena) of a factored input, cached; the solve options are left off by whoever sets them (deterministic())."""
    if name not in _DEV:
        _DEV[name] = factored(ca, S.plan)
    return _DEV[name]


@contextlib.contextmanager
def deterministic(dev, on=True):
    """Both deterministic solve options for the body."""
    for opt in ("solve_deterministic", "solve_deterministic_block"):
        dev.set_option(opt, 1 if on else 0)
    try:
        yield
    finally:
        for opt in ("solve_deterministic", "solve_deterministic_block"):
            dev.set_option(opt, 0)


def block(V, ld=None):
    """An n x k Guarded block holding V (column-major, leading dimension ld, default rows + 3)."""
    return Guarded(V.shape[0], V.shape[1], V.shape[0] + 3 if ld is None else ld, values=V)


def vec(v):
    return Guarded(len(v), values=v)


def cases():
    """(input, mode, k, nrhs): every k of the list (capped at n) on every input in every mode, nrhs going round its list."""
    out = []
    for name in INPUTS:
        for mi, mode in enumerate((lr.UPDATE, lr.DOWNDATE, lr.CONSTRAINT)):
            for i, k in enumerate(lr.ks_of(SIZES[name])):
                out.append(pytest.param(name, mode, k, lr.NRHS[(i + mi) % len(lr.NRHS)], id=f"{name}-{MODE_IDS[mi]}-k{k}"))
    return out


def run_solves(low, a, B, E, inplace=False):
    """(x of column 0 by solve, X by solve_nrhs) through guarded blocks with ld = n + 3; guards, padding and inputs are checked."""
    n, nrhs = B.shape
    gb, gB = vec(B[:, 0]), block(B)
    ge = None if E is None else vec(E[:, 0])
    gE = None if E is None else block(E)
    snaps = [(g, g.snapshot()) for g in (gb, gB, ge, gE) if g is not None]
    gx, gX = (gb, gB) if inplace else (Guarded(n), Guarded(n, nrhs, n + 3))
    if inplace:
        snaps = snaps[2:]
    low.solve(a, gb.t, gx.t, e=None if ge is None else ge.t)
    low.solve_nrhs(a, gB.t, gX.t, E=None if gE is None else gE.t)
    low.dev.sync()
    for g, s in snaps:
        g.assert_unchanged(s, "an input of the corrected solve")
    gx.assert_guards("x")
    gX.assert_guards("X")
    return gx.numpy(), gX.numpy()


# ------------------------------------------------------------------------------------------------
# 1. set, solve, solve_nrhs, logdet, diag against the references: gates 3, 4, 5 and the constraint residual
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode,k,nrhs", cases())
def test_corrected_solve_logdet_and_diag(name, mode, k, nrhs, ca, spd):
    S = spd(name)
    assert S.n == SIZES[name]
    U, rs, B, E, Xref, np_ratio = lr.prepare(S, name, mode, k, nrhs)
    dev, a = device_of(ca, name, S)
    low = ca.LowRank(dev, k)
    gU = block(U)
    snap = gU.snapshot()
    low.set(a, gU.t, mode)
    gU.assert_unchanged(snap, "U")
    assert low.state() == (k, mode, 0)
    x, X = run_solves(low, a, B, E)
    gate = rs.gate4()
    r4 = max(lr.forward_error(S, x, Xref[:, 0]), lr.forward_error(S, X, Xref)) / gate
    r5 = abs(low.logdet_c() - rs.logdet_c) / rs.gate5()
    LC = low.factor()
    assert np.array_equal(LC, np.tril(LC)) and abs(2.0 * np.log(np.diag(LC)).sum() - low.logdet_c()) <= 2.0 * (k + 1) * U64 * np.abs(np.log(np.diag(LC))).sum()
    W = low.block()
    r3 = lr.gate3_ratio(low.diag().cpu().numpy(), W)
    rc = max(lr.constraint_ratio(rs, x, None if E is None else E[:, 0]), lr.constraint_ratio(rs, X, E)) if mode == lr.CONSTRAINT else 0.0
    rl = 0.0
    if mode == lr.UPDATE and k in (17, 256, S.n):                    # log det(A + U U^T) = log det A + log det C against the dense slogdet
        sign, ref = np.linalg.slogdet(S.A + U @ U.T)
        assert sign > 0
        rl = abs(dev.logdet(a) + low.logdet_c() - ref) / (logdet_tol(S) + rs.gate5())
    print(f"{name} mode {mode} k {k} nrhs {nrhs}: error / gate: solve {r4:.3e} (numpy restatement {np_ratio:.3e}), logdet C {r5:.3e}, diag {r3:.3e}, "
          f"constraint {rc:.3e}, logdet A' {rl:.3e}; kappa(C) = {rs.kappa_c:.2f}")
    assert r4 <= 1.0 and r5 <= 1.0 and r3 <= 1.0 and rc <= 1.0 and rl <= 1.0
    low.close()


def test_case_sizes_are_the_inputs_sizes(spd):
    assert {name: spd(name).n for name in INPUTS} == SIZES


def test_generic_gaussian_update(ca, spd):
    """Seeded Gaussian columns with no control of C: gate 4 with its own kappa_2(C_ref)."""
    name, k, nrhs = "lapl_400x400", 33, 33
    S = spd(name)
    U = lr.gaussian_u(S, k)
    rs = lr.Restated(S, U, lr.UPDATE)
    B = np.asfortranarray(S.s[:, None] * np.random.default_rng(11).standard_normal((S.n, nrhs)))
    Xref = lr.reference_solve(S, U, lr.UPDATE, B)
    np_ratio = lr.check_conditions(S, rs, B, Xref)
    dev, a = device_of(ca, name, S)
    low = ca.LowRank(dev, 64)                                         # kmax > k: the object's matrices have a leading dimension of their own
    low.set(a, block(U).t, "update")
    x, X = run_solves(low, a, B, None)
    r4 = max(lr.forward_error(S, x, Xref[:, 0]), lr.forward_error(S, X, Xref)) / rs.gate4()
    r5 = abs(low.logdet_c() - rs.logdet_c) / rs.gate5()
    print(f"generic update: kappa(C) = {rs.kappa_c:.3e}, solve error / gate {r4:.3e} (numpy {np_ratio:.3e}), logdet C {r5:.3e}")
    assert r4 <= 1.0 and r5 <= 1.0
    low.close()


# ------------------------------------------------------------------------------------------------
# 2. contracts
# ------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_repeatability(ca, spd):
    """Kernels 1-3 return the same bits call to call and from a second object; with both deterministic solve options set twice gives identical W, L_C,
    solve and solve_nrhs bits."""
    name, k, nrhs = "lapl_3375x3375", 33, 33
    S = spd(name)
    U, rs, B, E, Xref, _ = lr.prepare(S, name, lr.CONSTRAINT, k, nrhs)
    assert E is not None
    dev, a = device_of(ca, name, S)
    import torch
    x = torch.from_numpy(S.rhs.copy()).cuda()
    e = torch.from_numpy(E[:, 0].copy()).cuda()
    with deterministic(dev):
        lows, got = [ca.LowRank(dev, k), ca.LowRank(dev, 256)], []
        for low in lows + lows[:1]:
            low.set(a, block(U).t, lr.CONSTRAINT)
            xs, Xs = run_solves(low, a, B, E)
            got.append((low.block(), low.factor(), xs, Xs, low.logdet_c()))
        for g in got[1:]:
            for p, q in zip(got[0][:4], g[:4]):
                assert np.array_equal(bits(p), bits(q))
            assert g[4] == got[0][4]
    # the three kernels alone, whatever the solve options: rowsq (diag), tprod + rprod (project: U^T x, R^T t, x - W r)
    d = [low.diag().cpu().numpy() for low in lows + lows]
    pr = [low.project(block(U).t, x, e=e).cpu().numpy() for low in lows + lows]
    for q in d[1:]:
        assert np.array_equal(bits(d[0]), bits(q))
    for q in pr[1:]:
        assert np.array_equal(bits(pr[0]), bits(q))
    for low in lows:
        low.close()


def test_column_independence(ca, spd):
    """Column j of the correction X - X0 depends on column j of B and E alone: nrhs 1 against 33, a column moved between chunks, a NaN in a neighbour.
    The plain solve inside runs under the deterministic block options, whose X0 has the same property bit for bit."""
    name, k, nrhs = "lapl_3375x3375", 33, 33
    S = spd(name)
    U, rs, B, E, Xref, _ = lr.prepare(S, name, lr.CONSTRAINT, k, nrhs)
    dev, a = device_of(ca, name, S)
    low = ca.LowRank(dev, k)
    with deterministic(dev):
        low.set(a, block(U).t, lr.CONSTRAINT)

        def solve(Bm, Em):
            gX = Guarded(S.n, Bm.shape[1], S.n + 3)
            low.solve_nrhs(a, block(Bm).t, gX.t, E=block(Em).t)
            dev.sync()
            gX.assert_guards("X")
            return gX.numpy()

        X = solve(B, E)
        for j in (0, 5, 31, 32):
            assert np.array_equal(bits(solve(B[:, j:j + 1], E[:, j:j + 1])[:, 0]), bits(X[:, j])), j
        order = np.r_[32, 1:32, 0]                                     # column 0 moves to the second chunk, column 32 to the first
        Xm = solve(np.asfortranarray(B[:, order]), np.asfortranarray(E[:, order]))
        assert np.array_equal(bits(Xm), bits(X[:, order]))
        Bn, En = B.copy(order="F"), E.copy(order="F")
        Bn[:, 4], En[:, 6], Bn[7, 20] = np.nan, np.nan, np.nan
        Xn = solve(Bn, En)
        clean = [j for j in range(nrhs) if j not in (4, 6, 20)]
        assert np.array_equal(bits(Xn[:, clean]), bits(X[:, clean]))
        assert all(np.isnan(Xn[:, j]).any() for j in (4, 6, 20))
    low.close()


def test_guarded_buffers_and_extra_columns(ca, spd):
    """Rows n .. ld - 1, columns >= nrhs and the guard tails are untouched (run_solves checks the first and the last in every test)."""
    name, k, nrhs = "tree_over", 33, 33
    S = spd(name)
    U, rs, B, E, Xref, _ = lr.prepare(S, name, lr.CONSTRAINT, k, nrhs)
    dev, a = device_of(ca, name, S)
    low = ca.LowRank(dev, k)
    low.set(a, block(U).t, lr.CONSTRAINT)
    for cols in (1, 31, 32, 33):
        gX = Guarded(S.n, nrhs + 2, S.n + 3)
        before = gX.snapshot()
        low.solve_nrhs(a, block(B[:, :cols]).t, gX.t[:, :cols], E=block(E[:, :cols]).t)
        dev.sync()
        gX.assert_guards("X")
        after = gX.bits()
        written = np.zeros(after.shape, dtype=bool)
        written[GUARD:GUARD + (S.n + 3) * (nrhs + 2)].reshape(nrhs + 2, S.n + 3)[:cols, :S.n] = True
        assert np.array_equal(after[~written], before[~written]), f"{cols} columns: something outside n x nrhs was written"
        assert lr.forward_error(S, gX.numpy()[:, :cols], Xref[:, :cols]) <= rs.gate4()
    gw = Guarded(S.n)
    low.diag(out=gw.t)
    gx = Guarded(S.n)
    low.project(block(U).t, vec(S.rhs).t, xout=gx.t, e=vec(E[:, 0]).t)
    dev.sync()
    gw.assert_guards("w")
    gx.assert_guards("xout")
    low.close()


@pytest.mark.parametrize("name", POISON_INPUTS)
def test_poisoned_scratch(name, ca, spd, monkeypatch):
    """Under CHOLAMD_POISON=1 (every library buffer NaN-filled, guard tails behind it) the results are finite and equal the unpoisoned run's to gate 4; with
    the deterministic options they are equal bit for bit."""
    S = spd(name)
    got = {}
    for poisoned in (False, True):
        if poisoned:
            monkeypatch.setenv("CHOLAMD_POISON", "1")
        dev, a = factored(ca, S.plan)
        for mode, k, nrhs in ((lr.UPDATE, 17, 33), (lr.CONSTRAINT, 70, 31)):
            U, rs, B, E, Xref, _ = lr.prepare(S, name, mode, k, nrhs)
            for det in (False, True):
                with deterministic(dev, det):
                    low = ca.LowRank(dev, 256)                        # kmax > k: the unused part of every matrix stays poisoned
                    low.set(a, block(U).t, mode)
                    x, X = run_solves(low, a, B, E)
                    w = low.diag().cpu().numpy()
                    got[poisoned, mode, det] = (x, X, low.block(), low.factor(), w)
                    low.close()
                assert all(np.all(np.isfinite(v)) for v in got[poisoned, mode, det])
                assert max(lr.forward_error(S, x, Xref[:, 0]), lr.forward_error(S, X, Xref)) <= rs.gate4()
                if poisoned:
                    assert lr.forward_error(S, X, got[False, mode, det][1]) <= rs.gate4()
        del dev, a
    monkeypatch.delenv("CHOLAMD_POISON")
    for (poisoned, mode, det), v in got.items():
        if poisoned and det:
            for p, q in zip(v, got[False, mode, True]):
                assert np.array_equal(bits(p), bits(q)), (mode, "the poisoned run's bits differ")


def test_in_place(ca, spd):
    """x == b and X == B (equal leading dimensions) equal the out-of-place calls: t = W^T b is taken before the plain solve overwrites b."""
    name = "lapl_400x400"
    S = spd(name)
    dev, a = device_of(ca, name, S)
    for mode, k, nrhs in ((lr.DOWNDATE, 32, 33), (lr.CONSTRAINT, 17, 32)):
        U, rs, B, E, Xref, _ = lr.prepare(S, name, mode, k, nrhs)
        low = ca.LowRank(dev, k)
        with deterministic(dev):
            low.set(a, block(U).t, mode)
            x0, X0 = run_solves(low, a, B, E)
            x1, X1 = run_solves(low, a, B, E, inplace=True)
        assert np.array_equal(bits(x0), bits(x1)) and np.array_equal(bits(X0), bits(X1))
        x2, X2 = run_solves(low, a, B, E, inplace=True)               # and on the atomic path to the gate
        assert max(lr.forward_error(S, x2, Xref[:, 0]), lr.forward_error(S, X2, Xref)) <= rs.gate4()
        low.close()


def test_failure_paths(ca, spd):
    name = "lapl_400x400"
    S = spd(name)
    n = S.n
    dev, a = device_of(ca, name, S)
    L = dev.L
    low = ca.LowRank(dev, 33)
    import torch
    b, x = torch.from_numpy(S.rhs.copy()).cuda(), torch.full((n,), 7.0, dtype=torch.float64, device="cuda")

    def refused(what):
        """Every use of the unset object: CHOLAMD_ERR_ARG and nothing written."""
        out = C.c_double(5.0)
        p, ld = C.c_void_p(), C.c_int64(0)
        h = np.full(4, 5.0)
        P = ca.Device.ptr
        assert L.cholamd_lowrank_solve(low.h, P(a), P(b), None, P(x), None) == ERR_ARG, what
        assert L.cholamd_lowrank_solve_nrhs(low.h, P(a), P(b), n, None, 33, P(x), n, 1, None) == ERR_ARG, what
        assert L.cholamd_lowrank_project(low.h, P(b), n, P(b), None, P(x), None) == ERR_ARG, what
        assert L.cholamd_lowrank_diag(low.h, P(x), None) == ERR_ARG, what
        assert L.cholamd_lowrank_logdet(low.h, C.byref(out)) == ERR_ARG and out.value == 5.0, what
        assert L.cholamd_lowrank_factor(low.h, h.ctypes.data, 2) == ERR_ARG and np.all(h == 5.0), what
        assert L.cholamd_lowrank_block(low.h, C.byref(p), C.byref(ld)) == ERR_ARG and p.value is None, what
        assert b"unset" in L.cholamd_last_error()
        dev.sync()
        assert torch.all(x == 7.0), what

    assert low.state() == (0, 0, 0)
    refused("a fresh object")
    # a downdate too large: c = 2 puts every eigenvalue of G above 1
    U = lr.build_u(S, 17, lr.DOWNDATE, c=2.0)
    with pytest.raises(ca.CholamdError, match="not positive definite at leading minor"):
        low.set(a, block(U).t, lr.DOWNDATE)
    k, mode, info = low.state()
    assert k == 0 and mode == lr.DOWNDATE and 1 <= info <= 17
    refused("after a failed downdate")
    # a constraint block with an exactly zero column j: info == j + 1
    for j in (0, 16, 32):
        U = lr.build_u(S, 33, lr.CONSTRAINT)
        U[:, j] = 0.0
        with pytest.raises(ca.CholamdError, match="dependent or zero"):
            low.set(a, block(U).t, lr.CONSTRAINT)
        assert low.state() == (0, lr.CONSTRAINT, j + 1)
    refused("after a zero constraint column")
    # argument errors: the object keeps the state it had (here: set)
    U = lr.build_u(S, 33, lr.UPDATE)
    gU = block(U)
    low.set(a, gU.t, lr.UPDATE)
    P = ca.Device.ptr
    bad = [(P(a), P(gU), n + 3, 0, 1), (P(a), P(gU), n + 3, 34, 1), (P(a), P(gU), n - 1, 33, 1), (None, P(gU), n + 3, 33, 1), (P(a), None, n + 3, 33, 1),
           (P(a), P(gU), n + 3, 33, 2), (P(a), P(gU), n + 3, 33, -2)]
    for arena, u, ldu, k, mode in bad:
        assert L.cholamd_lowrank_set(low.h, arena, u, ldu, k, mode, None) == ERR_ARG, (ldu, k, mode)
        assert low.state() == (33, lr.UPDATE, 0)
    assert L.cholamd_lowrank_set(None, P(a), P(gU), n + 3, 33, 1, None) == ERR_ARG
    h = C.c_void_p()
    for kmax in (0, -1, 257):
        assert L.cholamd_lowrank_create(dev.h, kmax, C.byref(h)) == ERR_ARG and h.value is None
    assert L.cholamd_lowrank_create(None, 4, C.byref(h)) == ERR_ARG and L.cholamd_lowrank_create(dev.h, 4, None) == ERR_ARG
    # solve_nrhs: the argument rules of cholamd_solve_nrhs
    X = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    assert L.cholamd_lowrank_solve_nrhs(low.h, P(a), P(b), n, None, 33, P(X), n, 0, None) == 0
    assert L.cholamd_lowrank_solve_nrhs(low.h, None, None, n, None, 33, None, n, 0, None) == 0
    for args in [(P(a), P(b), n, None, 33, P(X), n, -1), (P(a), P(b), n - 1, None, 33, P(X), n, 1), (P(a), P(b), n, None, 33, P(X), n - 1, 1),
                 (None, P(b), n, None, 33, P(X), n, 1), (P(a), None, n, None, 33, P(X), n, 1), (P(a), P(b), n, None, 33, None, n, 1)]:
        assert L.cholamd_lowrank_solve_nrhs(low.h, *args, None) == ERR_ARG, args
    assert L.cholamd_lowrank_project(low.h, P(gU), n + 3, P(b), None, P(X), None) == ERR_ARG      # not in constraint mode
    dev.sync()
    assert torch.all(X == 7.0)
    low.close()
    # a partitioned device object of rank != 0 holds no complete factor
    dev2 = ca.Device(S.plan, 0)
    dev2.set_partition(1, 2)
    assert L.cholamd_lowrank_create(dev2.h, 4, C.byref(h)) == ERR_ARG and h.value is None
    dev2.set_partition(0, 1)
    low2 = ca.LowRank(dev2, 4)
    dev2.set_partition(1, 2)
    assert L.cholamd_lowrank_set(low2.h, P(a), P(gU), n + 3, 4, 1, None) == ERR_ARG and low2.state()[0] == 0
    low2.close()


def test_no_leaks(ca, spd):
    name = "lapl_25x25"
    S = spd(name)
    dev, a = device_of(ca, name, S)
    U, rs, B, E, Xref, _ = lr.prepare(S, name, lr.UPDATE, 17, 33)
    warm = ca.LowRank(dev, 17)                                        # what the device object itself allocates at its first solves stays with it
    warm.set(a, block(U).t, lr.UPDATE)
    run_solves(warm, a, B, None)
    warm.close()
    live = dev.L.cholamd_debug_live_buffers()
    low = ca.LowRank(dev, 25)
    assert dev.L.cholamd_debug_live_buffers() == live + 6
    low.set(a, block(U).t, lr.UPDATE)
    run_solves(low, a, B, None)
    low.diag()
    bad = lr.build_u(S, 17, lr.DOWNDATE, c=2.0)
    with pytest.raises(ca.CholamdError):
        low.set(a, block(bad).t, lr.DOWNDATE)
    low.close()
    assert dev.L.cholamd_debug_live_buffers() == live


@pytest.mark.parametrize("name,k", [("lapl_25x25", 16), ("lapl_3375_scaled", 33), ("tree_over", 70)])
def test_project(name, k, ca, spd):
    """x* = x - W L_C^-1 (U^T x - e): U^T x* = e to the constraint gate, x* equals the numpy formula to gate 4."""
    S = spd(name)
    U, rs, B, E, Xref, _ = lr.prepare(S, name, lr.CONSTRAINT, k, 33 if k == 33 else lr.NRHS[(lr.ks_of(S.n).index(k) + 2) % 4])
    dev, a = device_of(ca, name, S)
    low = ca.LowRank(dev, k)
    low.set(a, block(U).t, lr.CONSTRAINT)
    rng = np.random.default_rng(k)
    x = rs.plain(S.rhs[:, None])[:, 0] + rng.standard_normal(S.n) / S.s        # a sample around the mean: mu + M^-T z would do as well
    e = 0.5 * (U.T @ x)
    worst = 0.0
    for ev in (e, None):
        ref = rs.project(x, ev)
        gx = vec(x)
        out = low.project(block(U).t, gx.t, xout=Guarded(S.n).t, e=None if ev is None else vec(ev).t).cpu().numpy()
        low.project(block(U).t, gx.t, xout=gx.t, e=None if ev is None else vec(ev).t)       # in place
        dev.sync()
        gx.assert_guards("x")
        assert np.array_equal(bits(gx.numpy()), bits(out))
        r4 = lr.forward_error(S, out, ref) / rs.gate4()
        rc = lr.constraint_ratio(rs, out, ev)
        worst = max(worst, r4, rc)
        print(f"{name} k {k} e {'given' if ev is not None else 'zero'}: x* error / gate 4 = {r4:.3e}, |U^T x* - e| / gate = {rc:.3e}")
    assert worst <= 1.0
    low.close()
