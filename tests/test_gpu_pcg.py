"""cholamd_apply and cholamd_solve_pcg on the GPU: conjugate gradients on the values IN FORCE (A'), preconditioned with the factor of the values the arena
was factored from (A).  A' is applied by set_values with no refactorisation; the arenas (fp64 and fp32) hold the factor of A throughout.

The iteration caps come from tests/pcg_ref.py (the numpy loop, which tests/test_pcg_host.py holds to the same caps on the same inputs) and from exact
arithmetic: one step for A' = 3 A (cap 2), m + 1 for a change of rank m (cap m + 2), the classical bound for a diagonal drift.  On lapl_9x9 and
lapl_25x25 the reference itself needs m + 2 = 10 steps at m = 8 (eight outlying eigenvalues in a space of 9 or 25 dimensions: the ninth step leaves
1e-10 .. 1e-9), so the cap has no slack there, and those two cases run under solve_deterministic: their count is the same on every run.  All caller buffers are guarded.Guarded blocks with ld = n + 3."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pcg_ref as pr  # noqa: E402
from conftest import ROOT  # noqa: E402
from guarded import Guarded  # noqa: E402
from pcg_ref import MAX_ITER, TOL  # noqa: E402

nrhs_of = pr.nrhs_of
_CTX = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module", autouse=True)
def release_devices():
    """The device objects, their arenas and workspaces live for this module only: nothing of them stays allocated for the tests that follow."""
    yield
    import gc
    import torch
    _CTX.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def ctx(tmp_path_factory, name):
    """(S, device object, fp64 arena, fp32 arena): both arenas hold the factor of S's own values A, made before any set_values."""
    if name not in _CTX:
        import cholesky_amd as ca
        S = pr.spd(tmp_path_factory, name)
        dev = ca.Device(S.plan, 0)
        a64, a32 = dev.new_arena(), dev.new_arena_f32()
        dev.fill(a64)
        dev.factor(a64)
        dev.sync()
        assert dev.info() == (0, 0)
        dev.fill_f32(a32)
        dev.factor_f32(a32)
        dev.sync()
        assert dev.info() == (0, 0)
        _CTX[name] = (S, dev, a64, a32)
    return _CTX[name]


def set_values(dev, vals):
    g = Guarded(len(vals), values=vals)
    snap = g.snapshot()
    dev.set_values(g.t)
    dev.sync()
    g.assert_unchanged(snap, "value array")


def run(dev, arena, B, x0=None, single=False, **kw):
    """solve_pcg_nrhs (single: solve_pcg on the one column) on guarded blocks with ld = n + 3; returns (X, iters, relres, status) as arrays.
    X starts as NaN unless x0 is given; B and every guard must come back untouched."""
    n, k = B.shape
    start = np.full((n, k), np.nan) if x0 is None else x0
    if single:
        assert k == 1
        Bg, Xg = Guarded(n, values=B[:, 0]), Guarded(n, values=start[:, 0])
    else:
        Bg, Xg = Guarded(n, k, ld=n + 3, values=B), Guarded(n, k, ld=n + 3, values=start)
    snap = Bg.snapshot()
    try:
        if single:
            it, rel, st = dev.solve_pcg(arena, Bg.t, Xg.t, x0=x0 is not None, **kw)
            it, rel, st = np.array([it]), np.array([rel]), np.array([st])
        else:
            it, rel, st = dev.solve_pcg_nrhs(arena, Bg.t, Xg.t, x0=x0 is not None, **kw)
    except Exception as e:  # a refused or failed call: what it left in X travels with the exception
        dev.sync()
        e.X = Xg.numpy().reshape(n, k)
        raise
    finally:
        dev.sync()
        Bg.assert_unchanged(snap, "B")
        Xg.assert_guards("X")
    return Xg.numpy().reshape(n, k), it, rel, st


def check_columns(case, X, B, rel):
    """case 5 of the issue on every column"""
    kappa = case.kappa2()
    for j in range(B.shape[1]):
        case.check_converged(X[:, j], B[:, j], rel[j], kappa=kappa)


# ---- 1. apply ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pr.GPU_INPUTS)
def test_apply_equals_the_host_bit_for_bit(tmp_path_factory, name):
    S, dev, _, _ = ctx(tmp_path_factory, name)
    n, k = S.n, nrhs_of(name)
    rng = np.random.default_rng(5)
    X = rng.standard_normal((n, k)) / S.s[:, None]
    import cholesky_amd as ca
    fresh = ca.Device(S.plan, 0)  # no set_values yet: the operator is the plan's own upload
    for dev, vals in ((fresh, None), (dev, pr.values(S)), (dev, pr.drift(S).vals)):
        if vals is not None:
            set_values(dev, vals)
        Xg, Yg = Guarded(n, k, ld=n + 3, values=X), Guarded(n, k, ld=n + 5)
        xg, yg = Guarded(n, values=X[:, 0]), Guarded(n)
        snaps = Xg.snapshot(), xg.snapshot()
        dev.apply_nrhs(Xg.t, Yg.t)
        dev.apply(xg.t, yg.t)
        dev.sync()
        Xg.assert_unchanged(snaps[0], "X")
        xg.assert_unchanged(snaps[1], "x")
        Yg.assert_guards("Y")
        yg.assert_guards("y")
        want = np.stack([S.plan.apply_host(X[:, j], values=vals) for j in range(k)], axis=1)
        assert np.array_equal(bits(Yg.numpy()), bits(want))
        assert np.array_equal(bits(yg.numpy()), bits(want[:, 0]))


# ---- 2. A' = 3 A ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pr.GPU_INPUTS)
def test_scaled_values_take_one_step(tmp_path_factory, name):
    S, dev, a64, a32 = ctx(tmp_path_factory, name)
    case = pr.scaled(S)
    set_values(dev, case.vals)
    k = nrhs_of(name)
    B = case.rhs(k)
    X, it, rel, st = run(dev, a64, B, max_iter=MAX_ITER, tol=TOL)
    print(f"{name}: fp64 arena, iters {it.tolist()}, relres max {rel.max():.2e}")
    assert (st == 0).all() and (it <= 2).all(), (it, st)
    check_columns(case, X, B, rel)
    ref32 = [case.pcg(B[:, j], f32=True)[1] for j in range(k)]
    X, it, rel, st = run(dev, a32, B, max_iter=MAX_ITER, tol=TOL)
    print(f"{name}: fp32 arena, iters {it.tolist()}, reference {ref32}")
    assert (st == 0).all() and (it <= np.array(ref32) + 1).all(), (it, ref32, st)
    check_columns(case, X, B, rel)
    # the contrast: the stationary refinement on the same arena and values has the iteration matrix -2 I
    import cholesky_amd as ca
    import torch
    d_b, d_x = torch.from_numpy(B[:, 0].copy()).cuda(), torch.zeros(S.n, dtype=torch.float64, device="cuda")
    try:
        _, rr = dev.solve_refine(a32, d_b, d_x, max_iter=20, tol=TOL)
    except ca.CholamdError:
        rr = float("nan")
    print(f"{name}: solve_refine after 20 corrections: {rr:.2e}")
    assert not rr <= TOL


# ---- 3. a change of rank m ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 3, 8])
@pytest.mark.parametrize("name", pr.GPU_INPUTS)
def test_rank_m_change_takes_m_plus_one_steps(tmp_path_factory, name, m):
    S, dev, a64, _ = ctx(tmp_path_factory, name)
    case, B = pr.rank_inputs(S, name, m)
    set_values(dev, case.vals)
    # where the reference itself leaves the cap no slack, the reproducible solve: the count is then the same on every run
    tight = m == 8 and name in ("lapl_9x9", "lapl_25x25")
    try:
        det_options(dev, tight, False)
        X, it, rel, st = run(dev, a64, B, max_iter=MAX_ITER, tol=TOL)
    finally:
        det_options(dev, False, False)
    print(f"{name}, m = {m}: iters {it.tolist()}, relres max {rel.max():.2e}")
    assert (st == 0).all() and (it <= m + 2).all(), (it, st)
    check_columns(case, X, B, rel)


# ---- 4. / 6. drift, and the start vector --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pr.GPU_INPUTS + [pr.BIG])
def test_drift_meets_the_classical_bound(tmp_path_factory, name):
    S, dev, a64, a32 = ctx(tmp_path_factory, name)
    case = pr.drift(S)
    k = pr.drift_nrhs(name)
    B = case.rhs(k)
    bound = case.drift_bound()
    ref = np.array([case.pcg(B[:, j])[1] for j in range(k)])
    set_values(dev, pr.values(S))
    X_prev = run(dev, a64, B, max_iter=MAX_ITER, tol=TOL)[0]  # the previous step's solution: A itself, one step
    set_values(dev, case.vals)
    X, it, rel, st = run(dev, a64, B, max_iter=MAX_ITER, tol=TOL)
    print(f"{name}: kp = {case.kp():.2f}, bound {bound}, reference {ref.tolist()}, iters {it.tolist()}, relres max {rel.max():.2e}")
    assert (st == 0).all() and (it <= np.minimum(ref + 1, bound)).all(), (it, ref, bound, st)
    check_columns(case, X, B, rel)
    Xs = np.stack([case.x_star(B[:, j]) for j in range(k)], axis=1)
    Xw, itw, relw, stw = run(dev, a64, B, x0=Xs, max_iter=MAX_ITER, tol=TOL)
    assert (itw == 0).all() and (stw == 0).all() and (relw <= TOL).all() and np.array_equal(bits(Xw), bits(Xs))
    Xw, itw, relw, stw = run(dev, a64, B, x0=X_prev, max_iter=MAX_ITER, tol=TOL)
    assert (stw == 0).all() and (itw <= it).all(), (itw, it)
    if name != pr.BIG:  # the fp32 arena of A as the preconditioner of A'
        X, it32, rel, st = run(dev, a32, B, max_iter=MAX_ITER, tol=TOL)
        assert (st == 0).all(), (it32, st)
        check_columns(case, X, B, rel)


# ---- 7. determinism and independence -----------------------------------------------------------------------------------------------------------------
def det_options(dev, det, block):
    dev.set_option("solve_deterministic", int(det))
    dev.set_option("solve_deterministic_block", int(block))


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", ["g17x15", "lapl_400x400", "tree_over"])
def test_deterministic_bits_and_independent_columns(tmp_path_factory, name, f32):
    S, dev, a64, a32 = ctx(tmp_path_factory, name)
    arena = a32 if f32 else a64
    case = pr.drift(S)
    set_values(dev, case.vals)
    B = case.rhs(33, seed=3)
    try:
        det_options(dev, True, False)
        r1 = run(dev, arena, B[:, :5], max_iter=MAX_ITER, tol=TOL)
        r2 = run(dev, arena, B[:, :5], max_iter=MAX_ITER, tol=TOL)
        for a, b in zip(r1, r2):
            assert np.array_equal(bits(a.astype(np.float64)), bits(b.astype(np.float64)))
        assert (r1[3] == 0).all()
        for j in (0, 4):  # a block column = the one-vector call on it
            s = run(dev, arena, B[:, j:j + 1], single=True, max_iter=MAX_ITER, tol=TOL)
            assert np.array_equal(bits(s[0][:, 0]), bits(r1[0][:, j])) and s[1][0] == r1[1][j] and s[2][0] == r1[2][j] and s[3][0] == 0
        det_options(dev, True, True)
        full = run(dev, arena, B, max_iter=MAX_ITER, tol=TOL)
        again = run(dev, arena, B, max_iter=MAX_ITER, tol=TOL)
        assert (full[3] == 0).all()
        for a, b in zip(full, again):
            assert np.array_equal(bits(a.astype(np.float64)), bits(b.astype(np.float64)))
        one = run(dev, arena, B[:, 32:33], max_iter=MAX_ITER, tol=TOL)  # nrhs 1 against 33; column 32 moves from the second chunk to the first
        assert np.array_equal(bits(one[0][:, 0]), bits(full[0][:, 32])) and one[1][0] == full[1][32] and one[2][0] == full[2][32]
        moved = run(dev, arena, B[:, [32] + list(range(1, 32)) + [0]], max_iter=MAX_ITER, tol=TOL)
        assert np.array_equal(bits(moved[0][:, 0]), bits(full[0][:, 32])) and np.array_equal(bits(moved[0][:, 32]), bits(full[0][:, 0]))
        assert moved[1][0] == full[1][32] and moved[1][32] == full[1][0]
        import cholesky_amd as ca
        Bn = B[:, :5].copy()
        Bn[S.n // 3, 2] = np.nan  # NaN in the neighbouring column
        with pytest.raises(ca.CholamdError, match="column 2 produced NaN") as e:
            run(dev, arena, Bn, max_iter=MAX_ITER, tol=TOL)
        assert e.value.status.tolist() == [0, 0, 3, 0, 0]
        ok = [0, 1, 3, 4]
        assert np.array_equal(e.value.iters[ok], full[1][ok]) and np.array_equal(bits(e.value.relres[ok]), bits(full[2][ok]))
        assert np.array_equal(bits(e.value.X[:, ok]), bits(full[0][:, ok]))
    finally:
        det_options(dev, False, False)


# ---- 8. failure paths --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lapl_25x25", "lapl_400x400", "tree_over"])
def test_failure_paths(tmp_path_factory, name):
    import cholesky_amd as ca
    import torch
    S, dev, a64, a32 = ctx(tmp_path_factory, name)
    L, n = dev.L, S.n
    case = pr.drift(S)
    set_values(dev, case.vals)
    B = case.rhs(3, seed=8)
    run(dev, a64, B, max_iter=MAX_ITER, tol=TOL)  # (every workspace exists from here on)
    # rank 1 of a partitioned object holds no complete factor
    d1 = ca.Device(S.plan, 0)
    d1.set_partition(1, 2)
    Bg, Xg = Guarded(n, 3, ld=n + 3, values=B), Guarded(n, 3, ld=n + 3)
    snap = Bg.snapshot()
    with pytest.raises(ca.CholamdError, match="rank 1 of 2"):
        d1.solve_pcg_nrhs(a64, Bg.t, Xg.t)
    d1.sync()
    Bg.assert_unchanged(snap, "B after the refused rank-1 call")
    Xg.assert_guards("X after the refused rank-1 call")
    assert np.isnan(Xg.t.cpu().numpy()).all()
    del d1
    live = L.cholamd_debug_live_buffers()
    # max_iter = 0: the start vector comes back with its true residual, status 1, return code 0
    X, it, rel, st = run(dev, a64, B, max_iter=0, tol=TOL)
    assert (it == 0).all() and (st == 1).all() and (X == 0).all() and (rel == 1.0).all()
    # zero b in the middle column, also under x0
    Bz = B.copy()
    Bz[:, 1] = 0.0
    for x0 in (None, np.ones((n, 3))):
        X, it, rel, st = run(dev, a64, Bz, x0=x0, max_iter=MAX_ITER, tol=TOL)
        assert (st == 0).all() and it[1] == 0 and rel[1] == 0.0 and (X[:, 1] == 0).all() and (it[[0, 2]] > 0).all()
    # x == b (in place)
    Xg = Guarded(n, 3, ld=n + 3, values=B)
    it, rel, st = dev.solve_pcg_nrhs(a64, Xg.t, Xg.t, max_iter=MAX_ITER, tol=TOL)
    dev.sync()
    Xg.assert_guards("X == B")
    assert (st == 0).all()
    check_columns(case, Xg.numpy(), B, rel)
    # an indefinite A': breakdown, x keeps the last iterate, the message names the column and the quantity
    bad, row = pr.indefinite(S)
    set_values(dev, bad.vals)
    Be = np.zeros((n, 3))
    Be[row, 1] = 1.0
    with pytest.raises(ca.CholamdError, match=r"column 1 broke down after \d+ iterations: p\^T A p = -") as e:
        run(dev, a64, Be, max_iter=MAX_ITER, tol=TOL)
    assert e.value.status.tolist() == [0, 2, 0] and np.isfinite(e.value.relres[1]) and np.isfinite(e.value.X).all()
    with pytest.raises(ca.CholamdError, match="broke down"):
        run(dev, a64, Be[:, 1:2], single=True, max_iter=MAX_ITER, tol=TOL)
    set_values(dev, case.vals)
    # argument errors: nothing is written
    Bg, Xg = Guarded(n, 3, ld=n + 3, values=B), Guarded(n, 3, ld=n + 3)
    p = lambda t: ca.Device.ptr(t)  # noqa: E731
    i3, r3 = np.full(3, -7, dtype=np.int32), np.full(3, -7.0)
    out = (i3.ctypes.data, r3.ctypes.data, i3.ctypes.data, None)
    for args, word in (((dev.h, p(a64), p(Bg.t), n - 1, p(Xg.t), n + 3, 3, 5, TOL, 0), "leading dimensions"),
                       ((dev.h, p(a64), p(Bg.t), n + 3, p(Xg.t), n + 3, -1, 5, TOL, 0), "nrhs = -1"),
                       ((dev.h, None, p(Bg.t), n + 3, p(Xg.t), n + 3, 3, 5, TOL, 0), "NULL arena"),
                       ((dev.h, p(a64), None, n + 3, p(Xg.t), n + 3, 3, 5, TOL, 0), "NULL B"),
                       ((dev.h, p(a64), p(Bg.t), n + 3, None, n + 3, 3, 5, TOL, 0), "NULL X"),
                       ((dev.h, p(a64), p(Bg.t), n + 3, p(Xg.t), n + 3, 3, 5, TOL, 2), "bad flags"),
                       ((dev.h, p(a64), p(Bg.t), n + 3, p(Xg.t), n + 3, 3, 5, -1.0, 0), "tol"),
                       ((dev.h, p(a64), p(Bg.t), n + 3, p(Xg.t), n + 3, 3, 5, float("nan"), 0), "tol")):
        for fn in (L.cholamd_solve_pcg_nrhs, L.cholamd_solve_pcg_nrhs_f32):
            assert fn(*args, *out) == -4
            assert word in L.cholamd_last_error().decode(), L.cholamd_last_error()
    assert L.cholamd_solve_pcg_nrhs(dev.h, p(a64), p(Bg.t), n + 3, p(Xg.t), n + 3, 0, 5, TOL, 0, *out) == 0  # nrhs = 0: nothing to do
    dev.sync()
    Xg.assert_guards("X after refused calls")
    assert np.isnan(Xg.t.cpu().numpy()).all() and (i3 == -7).all()
    for args, word in (((dev.h, None, n + 3, p(Xg.t), n + 3, 3, None), "NULL X"), ((dev.h, p(Bg.t), n + 3, None, n + 3, 3, None), "NULL Y"),
                       ((dev.h, p(Bg.t), n + 3, p(Bg.t), n + 3, 3, None), "overlaps"), ((dev.h, p(Bg.t), n + 3, p(Xg.t), n - 1, 3, None), "leading dimensions")):
        assert L.cholamd_apply_nrhs(*args) == -4
        assert word in L.cholamd_last_error().decode(), L.cholamd_last_error()
    dev.sync()
    Xg.assert_guards("Y after refused calls")
    assert np.isnan(Xg.t.cpu().numpy()).all()
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    with pytest.raises(ca.CholamdError, match="overlaps"):
        dev.apply(x, x)
    with pytest.raises(ca.CholamdError, match="NULL x"):
        check = ca._lib.check
        check(L.cholamd_apply(dev.h, None, p(x), None), "cholamd_apply")
    # repeated calls allocate nothing
    for _ in range(3):
        run(dev, a64, B, max_iter=MAX_ITER, tol=TOL)
        run(dev, a32, B[:, :1], single=True, max_iter=MAX_ITER, tol=TOL)
    assert L.cholamd_debug_live_buffers() == live


# ---- 9. poisoned workspaces, in a fresh process ------------------------------------------------------------------------------------------------------
class _Factory:
    def mktemp(self, name):
        import pathlib
        import tempfile
        return pathlib.Path(tempfile.mkdtemp(prefix=name))


def _det_run(name, f):
    """the deterministic block call of the drift case on `name`: (iters, status, relres, X)"""
    S, dev, a64, _ = ctx(f, name)
    case = pr.drift(S)
    set_values(dev, case.vals)
    B = case.rhs(5, seed=3)
    ref = np.array([case.pcg(B[:, j])[1] for j in range(5)])
    try:
        det_options(dev, True, True)
        X, it, rel, st = run(dev, a64, B, max_iter=MAX_ITER, tol=TOL)
    finally:
        det_options(dev, False, False)
    assert np.isfinite(X).all() and (st == 0).all() and (it <= np.minimum(ref + 1, case.drift_bound())).all(), (it, ref, st)
    check_columns(case, X, B, rel)
    return it, st, rel, X


def poison_child():
    assert os.environ.get("CHOLAMD_POISON") == "1"
    f = _Factory()
    for name in ("lapl_400x400", "tree_over"):
        it, st, rel, X = _det_run(name, f)
        print("poison", name, it.tolist(), bits(rel).tolist(), int(np.bitwise_xor.reduce(bits(X).ravel())))
    print("poison child ok")


def test_poisoned_workspaces(tmp_path_factory):
    env = dict(os.environ, CHOLAMD_POISON="1")
    code = f"import sys; sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); import conftest, test_gpu_pcg as t; t.poison_child()"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "poison child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("poison ")]
    for name, ln in zip(("lapl_400x400", "tree_over"), lines):
        it, st, rel, X = _det_run(name, tmp_path_factory)
        assert ln == " ".join(str(v) for v in ("poison", name, it.tolist(), bits(rel).tolist(), int(np.bitwise_xor.reduce(bits(X).ravel())))), ln
