"""Device.set_values: new values of A on a plan's pattern, from device memory, without a new plan.

The rule under test: after set_values(v) every entry point that takes the device object behaves as the same entry point of a device object
built on a plan created from the same entries with the values v.  Every comparison is therefore against a FRESH plan + device made from
the second matrix's own file (and against the CPU oracle / the dense references of that matrix), never against the object under test.

Inputs: spd_inputs' general SPD matrices; two seeds on one base give two matrices of one pattern (patterns "own" and "full" do not depend
on the seed).  A value array is the matrix's values in file order (spd_inputs.write_mtx sorts by (col, row)).  Tolerances are spd_inputs'
derived ones; fills are compared bit for bit.

The whole file runs twice: plainly, and with CHOLAMD_POISON=1 (every floating-point buffer the library allocates starts as NaN and has a
guard tail).  In both legs every value array is a guarded.Guarded view: the gather must read exactly nz doubles and write none of them."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import spd_inputs as si  # noqa: E402
from guarded import Guarded  # noqa: E402
from spd_inputs import U32, U64  # noqa: E402
from test_distributed import _assemble  # noqa: E402

MAX_ITER = 30
SECOND_SEED = 2000
_SECOND = {}


@pytest.fixture(autouse=True, params=[False, True], ids=["plain", "poison"])
def poison(request, monkeypatch):
    if request.param:
        monkeypatch.setenv("CHOLAMD_POISON", "1")
    else:
        monkeypatch.delenv("CHOLAMD_POISON", raising=False)
    return request.param


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """name -> (S1, S2): the suite's input `name` and a second matrix of another seed on the same pattern, each with its own plan and references."""
    def get(name):
        if name not in _SECOND:
            i = si.NAMES.index(name)
            _SECOND[name] = si.make(tmp_path_factory.mktemp(name + "_second"), name, seed=SECOND_SEED + i)
        S1, S2 = si.cached(tmp_path_factory, name), _SECOND[name]
        for a, b in zip(S1.plan.entries(), S2.plan.entries()):
            assert np.array_equal(a, b)
        return S1, S2
    return get


def order(S):
    return np.lexsort((S.row, S.col))


def values(S):
    """The value array of S: its values in the order of its matrix file."""
    return np.ascontiguousarray(S.val[order(S)])


def setv(dev, v, check=True):
    """dev.set_values from a guarded device array: the array is not written, its guards keep their bits."""
    g = Guarded(len(v), values=v)
    snap = g.snapshot()
    dev.set_values(g.t, check=check)
    dev.sync()
    g.assert_unchanged(snap, "value array")


def filled(dev, f32=False):
    a = Guarded(dev.plan.arena_doubles, dtype=_f32() if f32 else None)
    (dev.fill_f32 if f32 else dev.fill)(a.t)
    dev.sync()
    a.assert_guards("arena")
    out = a.t.cpu().numpy()
    assert np.isfinite(out).all()
    return out


def _f32():
    import torch
    return torch.float32


def factored(dev, f32=False):
    """(arena tensor, arena as fp64 numpy) filled and factored on dev."""
    a = dev.new_arena_f32() if f32 else dev.new_arena()
    (dev.fill_f32 if f32 else dev.fill)(a)
    (dev.factor_f32 if f32 else dev.factor)(a)
    dev.sync()
    assert dev.info() == (0, 0)
    out = a.cpu().numpy().astype(np.float64)
    assert np.isfinite(out).all()
    return a, out


def bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def dense(plan, arena):
    return np.tril(plan.arena_to_dense(np.asarray(arena, dtype=np.float64)))


def plan_with(tmp_path, S, vals, name):
    """A plan from S's entries in S's file order with the values `vals` (a file of its own)."""
    import cholesky_amd as ca
    o = order(S)
    path = os.path.join(str(tmp_path), name + ".mtx")
    si.write_mtx(path, S.n, S.row[o], S.col[o], vals)
    plan = ca.Plan(path, S.ord, S.clust)
    r, c = plan.entries()
    assert np.array_equal(r, S.row[o]) and np.array_equal(c, S.col[o])
    return plan


def sparse_of(S, vals):
    import scipy.sparse as sp
    o = order(S)
    r, c = S.row[o], S.col[o]
    off = r != c
    return sp.csr_matrix((np.concatenate([vals, vals[off]]), (np.concatenate([r, c[off]]), np.concatenate([c, r[off]]))), shape=(S.n, S.n))


# ------------------------------------------------------------------------------------------------
# a. fill
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lapl_400x400", "lapl_3375x3375", "g18_full"])
def test_fill_after_set_values_is_the_fresh_devices_fill(name, pair):
    import torch
    import cholesky_amd as ca
    S1, S2 = pair(name)
    v2 = values(S2)
    fresh = ca.Device(S2.plan, 0)
    dev = ca.Device(S1.plan, 0)
    before = filled(dev)
    assert not np.array_equal(before, filled(fresh))
    setv(dev, v2)
    assert dev.values_status() == (0, -1, 0, -1)
    for f32 in (False, True):
        assert np.array_equal(bits(filled(dev, f32)), bits(filled(fresh, f32))), f32
    assert np.array_equal(S1.plan.fill_host(), before)                 # the plan keeps its values
    # a host array (uploaded through the object's own buffer) and an unchecked call from a plain tensor: the same, and back again
    dev.set_values(values(S1))
    assert np.array_equal(bits(filled(dev)), bits(before))
    dev.set_values(torch.from_numpy(v2).cuda(), check=False)
    assert np.array_equal(bits(filled(dev)), bits(filled(fresh)))
    assert dev.values_status() == (0, -1, 0, -1)


@pytest.mark.parametrize("world,dist_top", [(2, 0), (2, 1), (4, 0), (4, 1)])
def test_partitioned_fill_and_factor_follow_set_values(world, dist_top, pair):
    """Rank objects over the local communicator: the owned-top copies of A's entries follow set_values -- when they exist at the call (a fill
    came first), when the schedule is rebuilt after it (set_option after set_values), and in the fp32 schedule's column blocks."""
    import torch
    import cholesky_amd as ca
    from cholesky_amd.device import factor_multi
    S1, S2 = pair("lapl_3375x3375")
    v2 = values(S2)

    def rank(plan, r, early):
        dev = ca.Device(plan, 0)
        if early:
            dev.set_option("dist_top", dist_top)
        dev.set_partition(r, world)
        return dev

    def arenas_of(devs, f32):
        out = []
        for dev in devs:
            a = torch.zeros(dev.plan.arena_doubles, dtype=torch.float32 if f32 else torch.float64, device="cuda")
            (dev.fill_f32 if f32 else dev.fill)(a)
            out.append(a)
        devs[0].sync()
        return out

    fresh = [rank(S2.plan, r, True) for r in range(world)]
    first = [rank(S1.plan, r, True) for r in range(world)]      # the top copies exist (a fill of matrix 1) when the values change
    for f32 in (False, True):
        old = arenas_of(first, f32)
        assert all(np.isfinite(a.cpu().numpy()).all() for a in old)
    late = [rank(S1.plan, r, False) for r in range(world)]      # the values change first, the schedule (and its top copies) afterwards
    for dev in first + late:
        setv(dev, v2)
    for dev in late:
        dev.set_option("dist_top", dist_top)
    for f32 in (False, True):
        ref = [a.cpu().numpy() for a in arenas_of(fresh, f32)]
        for devs in (first, late):
            got = [a.cpu().numpy() for a in arenas_of(devs, f32)]
            for r in range(world):
                assert np.array_equal(bits(got[r]), bits(ref[r])), (f32, r, devs is late)
    # the factorisation over the local communicator, against the fresh ranks' and the oracle's factor of matrix 2
    res = []
    for devs in (fresh, first):
        arenas = arenas_of(devs, False)
        factor_multi(devs, arenas, local=True)
        for dev in devs:
            assert dev.info() == (0, 0)
        parts = [a.cpu().numpy() for a in arenas]
        res.append(dense(S2.plan, _assemble(S2.plan, parts, world, parts[0])))
    assert np.isfinite(res[1]).all()
    assert S2.row_error(res[1], res[0]) <= S2.tol_factor()
    assert S2.row_error(res[1], S2.Lo) <= S2.tol_factor()


# ------------------------------------------------------------------------------------------------
# b. factor
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lapl_3375x3375", "g18_full"])   # the program launch; the level schedule
def test_factor_after_set_values_matches_fresh_device_and_oracle(name, pair):
    import cholesky_amd as ca
    S1, S2 = pair(name)
    dev = ca.Device(S1.plan, 0)
    _, first = factored(dev)                                     # the object has factored matrix 1 before
    assert S1.row_error(dense(S1.plan, first), S1.Lo) <= S1.tol_factor()
    setv(dev, values(S2))
    _, got = factored(dev)
    _, ref = factored(ca.Device(S2.plan, 0))
    L, Lf = dense(S1.plan, got), dense(S2.plan, ref)
    print(f"{name}: factor after set_values vs fresh device: bit for bit = {np.array_equal(bits(got), bits(ref))}, "
          f"row error {S2.row_error(L, Lf):.3e}, vs oracle {S2.row_error(L, S2.Lo):.3e}, tol {S2.tol_factor():.3e}")
    assert np.array_equal(L != 0, S2.Lo != 0)
    assert S2.row_error(L, Lf) <= S2.tol_factor()
    assert S2.row_error(L, S2.Lo) <= S2.tol_factor()


def test_five_value_sets_on_one_device_and_one_arena(tmp_path):
    """values -> fill -> factor -> solve and an 8-column block solve, five matrices in turn through ONE device object and ONE arena, each against
    its own references; then the first again: nothing of the four others survives."""
    import torch
    import cholesky_amd as ca
    _, base, opts = si.INPUTS[si.NAMES.index("g12_full")]
    sets = [si.SPD(str(tmp_path), base, 3000 + k, name=f"set{k}", oracle=False, **opts) for k in range(5)]
    dev = ca.Device(sets[0].plan, 0)
    arena = Guarded(dev.plan.arena_doubles)
    n = sets[0].n
    rng = np.random.default_rng(9)
    first = None
    for k in list(range(5)) + [0]:
        S = sets[k]
        setv(dev, values(S), check=k % 2 == 0)
        dev.fill(arena.t)
        dev.factor(arena.t)
        dev.sync()
        assert dev.info() == (0, 0)
        arena.assert_guards("arena")
        L = dense(dev.plan, arena.numpy())
        assert np.isfinite(L).all()
        assert S.row_error(L) <= S.tol_factor(), k
        if first is None:
            first = L
        elif k == 0:
            assert S.row_error(L, first) <= S.tol_factor()
        B = S.s[:, None] * rng.standard_normal((n, 8))
        B[:, 0] = S.rhs
        b, x = Guarded(n, values=B[:, 0]), Guarded(n)
        dev.solve(arena.t, b.t, x.t)
        dB, dX = Guarded(n, 8, values=B), Guarded(n, 8)
        dev.solve_nrhs(arena.t, dB.t, dX.t)
        dev.sync()
        x.assert_guards("x")
        dX.assert_guards("X")
        X = np.concatenate([x.numpy()[:, None], dX.numpy()], axis=1)
        for j in range(9):
            bj = B[:, max(j - 1, 0)]
            assert S.backward_error(X[:, j], bj) <= S.tol_backward(), (k, j)
            assert S.forward_error(X[:, j], S.reference_solve(bj)) <= S.tol_forward(), (k, j)


# ------------------------------------------------------------------------------------------------
# c. residual and refinement measure against the new A
# ------------------------------------------------------------------------------------------------
def _residual_bound(A, x, b):
    """|fl(b - A x) - (b - A x)| <= (m + 1) u (|A| |x| + |b|) componentwise for ANY order of a row's sum (m = the longest row), so two correctly
    rounded evaluations -- the device's and scipy's -- differ in ||r|| / ||b|| by at most (m + 1) u || |A| |x| + |b| || / ||b||."""
    m = int(np.diff(A.indptr).max())
    return (m + 1) * U64 * np.linalg.norm(abs(A) @ np.abs(x) + np.abs(b)) / np.linalg.norm(b)


@pytest.mark.parametrize("when", ["before_first_residual", "after_a_residual"])
def test_residual_follows_set_values(when, pair):
    import torch
    import cholesky_amd as ca
    S1, S2 = pair("lapl_3375x3375")
    b, x = S1.rhs, S1.x_ref                                      # x solves A1 x = b: the two residuals are orders of magnitude apart
    A1, A2 = S1.A_sparse, S2.A_sparse
    r1, r2 = (np.linalg.norm(b - A @ x) / np.linalg.norm(b) for A in (A1, A2))
    assert r2 > 1e6 * r1
    dev = ca.Device(S1.plan, 0)
    db, dx = Guarded(S1.n, values=b), Guarded(S1.n, values=x)
    if when == "after_a_residual":                               # the residual operator is on the device already
        got1 = dev.residual(db.t, dx.t)
        assert abs(got1 - r1) <= _residual_bound(A1, x, b)
    setv(dev, values(S2))
    got = dev.residual(db.t, dx.t)
    fresh = ca.Device(S2.plan, 0).residual(db.t, dx.t)
    print(f"{when}: device {got:.17g} scipy {r2:.17g} fresh {fresh:.17g} bound {_residual_bound(A2, x, b):.3e}")
    assert abs(got - r2) <= _residual_bound(A2, x, b)
    assert got == fresh
    setv(dev, values(S1))
    assert abs(dev.residual(db.t, dx.t) - r1) <= _residual_bound(A1, x, b)


def test_refinement_with_an_fp32_factor_of_the_new_matrix(pair):
    import cholesky_amd as ca
    S1, S2 = pair("lapl_3375x3375")
    dev = ca.Device(S1.plan, 0)
    a32, _ = factored(dev, f32=True)                             # an fp32 factor of matrix 1 first
    setv(dev, values(S2))
    a32, got = factored(dev, f32=True)
    assert S2.row_error(dense(S1.plan, got)) <= S2.tol_factor(U32)
    n, tol = S2.n, 1e-12
    b, x = Guarded(n, values=S2.rhs), Guarded(n)
    it, rel = dev.solve_refine(a32, b.t, x.t, max_iter=MAX_ITER, tol=tol)
    xs = x.numpy()
    assert rel <= tol and it <= S2.refine_iterations(tol), (it, rel, S2.refine_iterations(tol))
    true = S2.true_relres(xs, S2.rhs)
    assert abs(rel - true) <= 1e-13 + 0.5 * true
    assert S2.forward_error(xs) <= S2.tol_forward()
    rng = np.random.default_rng(3)
    B = S2.s[:, None] * rng.standard_normal((n, 8))
    dB, dX = Guarded(n, 8, values=B), Guarded(n, 8)
    it, rels = dev.solve_refine_nrhs(a32, dB.t, dX.t, max_iter=MAX_ITER, tol=tol)
    dX.assert_guards("X")
    X = dX.numpy()
    assert (rels <= tol).all() and it <= S2.refine_iterations(tol), (it, rels.max())
    for j in range(8):
        true = S2.true_relres(X[:, j], B[:, j])
        assert abs(rels[j] - true) <= 1e-13 + 0.5 * true
        assert S2.forward_error(X[:, j], S2.reference_solve(B[:, j])) <= S2.tol_forward(), j


# ------------------------------------------------------------------------------------------------
# d. refusals
# ------------------------------------------------------------------------------------------------
def test_out_of_pattern_values_are_refused_or_ignored(tmp_path, pair):
    import cholesky_amd as ca
    S1, S2 = pair("lapl_400x400")
    v1, v2 = values(S1), values(S2)
    o = order(S1)
    k = int(np.nonzero(S1.row[o] != S1.col[o])[0][123])
    z1, z2 = v1.copy(), v2.copy()
    z1[k] = z2[k] = 0.0
    plan = plan_with(tmp_path, S1, z1, "zero1")                  # entry k is in the list and outside the pattern
    assert plan.nnz_a == plan.nz - 1
    dev = ca.Device(plan, 0)
    before = filled(dev)
    with pytest.raises(ca.CholamdError, match=rf"entry {k} ") as e:
        setv(dev, v2)
    assert "code -4" in str(e.value)
    assert dev.values_status() == (0, -1, 1, k)
    for f32 in (False, True):                                    # the previous values are in force, in both precisions
        assert np.array_equal(bits(filled(dev, f32)), bits(filled(ca.Device(plan, 0), f32)))
    assert np.array_equal(bits(filled(dev)), bits(before))
    want = filled(ca.Device(plan_with(tmp_path, S1, z2, "zero2"), 0))
    setv(dev, v2, check=False)                                   # unchecked: the value is ignored and reported
    assert dev.values_status() == (0, -1, 1, k)
    assert np.array_equal(bits(filled(dev)), bits(want))
    setv(dev, z2)                                                # zero (and -0.0) there is what the pattern asks for
    assert dev.values_status() == (0, -1, 0, -1)
    assert np.array_equal(bits(filled(dev)), bits(want))
    z2[k] = -0.0
    setv(dev, z2)
    assert np.array_equal(bits(filled(dev)), bits(want))


@pytest.mark.parametrize("value", [1e39, 1e-39])
def test_fp32_range_refusal_follows_the_values(value, tmp_path, pair):
    import cholesky_amd as ca
    S1, S2 = pair("lapl_400x400")
    o = order(S2)
    r, c = S2.row[o], S2.col[o]
    # beyond FLT_MAX on the diagonal, below FLT_MIN off it: both matrices stay SPD (diagonally dominant)
    k = int(np.nonzero(r == c)[0][211]) if value > 1 else int(np.nonzero(r != c)[0][57])
    v = values(S2)
    v[k] = value
    dev = ca.Device(S1.plan, 0)
    a32 = dev.new_arena_f32()
    dev.fill_f32(a32)                                            # matrix 1 passes the range check: the verdict must not stick
    for check in (True, False):
        setv(dev, v, check=check)
        for fn in (dev.fill_f32, dev.factor_f32):
            with pytest.raises(ca.CholamdError, match=rf"entry {k} of A .*range") as e:
                fn(a32)
            assert "code -4" in str(e.value)
        assert dev.values_status() == (1, k, 0, -1)
        # fp64 has no such limit: factor and solve of the matrix with that entry
        a, got = factored(dev)
        ref = filled(ca.Device(plan_with(tmp_path, S2, v, f"range{int(check)}"), 0))
        assert np.array_equal(bits(filled(dev)), bits(ref))
        A = sparse_of(S2, v)
        b, x = Guarded(S2.n, values=S2.rhs), Guarded(S2.n)
        dev.solve(a, b.t, x.t)
        dev.sync()
        xs = x.numpy()
        be = (np.abs(S2.rhs - A @ xs) / (abs(A) @ np.abs(xs) + np.abs(S2.rhs))).max()
        assert be <= S2.tol_backward(), be
        setv(dev, values(S2), check=check)                       # sane values clear the refusal
        assert dev.values_status() == (0, -1, 0, -1)
        _, got32 = factored(dev, f32=True)
        assert S2.row_error(dense(S1.plan, got32)) <= S2.tol_factor(U32)


def test_explicit_zero_and_nan_in_the_pattern(tmp_path, pair):
    import cholesky_amd as ca
    S1, S2 = pair("lapl_400x400")
    o = order(S2)
    k = int(np.nonzero(S2.row[o] != S2.col[o])[0][300])
    v = values(S2)
    v[k] = 0.0                                                   # stored and factored as an explicit zero, on both precisions
    plan0 = plan_with(tmp_path, S2, v, "inzero")                 # (a plan made with it has the entry outside its pattern: the same arena)
    dev = ca.Device(S1.plan, 0)
    setv(dev, v)
    assert dev.values_status() == (0, -1, 0, -1)
    fresh = ca.Device(plan0, 0)
    for f32 in (False, True):
        assert np.array_equal(bits(filled(dev, f32)), bits(filled(fresh, f32)))
        _, got = factored(dev, f32)
        _, ref = factored(fresh, f32)
        u = U32 if f32 else U64
        assert S2.row_error(dense(S1.plan, got), dense(plan0, ref)) <= S2.tol_factor(u)
    # NaN: not refused, reaches the pivot checks of the fp64 factor as for a plan created with it
    v = values(S2)
    v[k] = np.nan
    for check in (True, False):
        setv(dev, v, check=check)
        assert dev.values_status() == (1, k, 0, -1)
        a = dev.new_arena()
        dev.fill(a)
        dev.factor(a)
        dev.sync()
        assert dev.info()[0] > 0
    setv(dev, values(S2))
    _, got = factored(dev)
    assert S2.row_error(dense(S1.plan, got), S2.Lo) <= S2.tol_factor()


# ------------------------------------------------------------------------------------------------
# e. ownership and arguments
# ------------------------------------------------------------------------------------------------
def test_two_device_objects_on_one_plan_keep_their_own_values(pair):
    import cholesky_amd as ca
    S1, S2 = pair("lapl_3375x3375")
    d1, d2 = ca.Device(S1.plan, 0), ca.Device(S1.plan, 0)
    setv(d2, values(S2))
    fresh1, fresh2 = filled(ca.Device(S1.plan, 0)), filled(ca.Device(S2.plan, 0))
    assert np.array_equal(bits(filled(d1)), bits(fresh1))
    assert np.array_equal(bits(filled(d2)), bits(fresh2))
    with pytest.raises(ca.CholamdError, match="no cholamd_device_set_values call"):
        d1.values_status()
    db, dx = Guarded(S1.n, values=S1.rhs), Guarded(S1.n, values=S1.x_ref)
    assert d2.residual(db.t, dx.t) > 1e6 * d1.residual(db.t, dx.t)


def test_arguments(pair):
    import torch
    import cholesky_amd as ca
    S1, S2 = pair("lapl_400x400")
    dev = ca.Device(S1.plan, 0)
    before = filled(dev)
    nz = S1.plan.nz
    good = torch.from_numpy(values(S2)).cuda()
    bad = [good.float(), good[:-1], torch.cat([good, good[:1]]), good.cpu(), torch.cat([good, good])[::2], good.reshape(1, -1),
           values(S2).astype(np.float32), values(S2)[:-1], np.concatenate([values(S2), values(S2)])[::2], list(values(S2)), None]
    for t in bad:
        with pytest.raises(ValueError):
            dev.set_values(t)
    L, ptr = dev.L, C.c_void_p(good.data_ptr())
    assert L.cholamd_device_set_values(dev.h, ptr, nz - 1, 0, None) == -4
    assert L.cholamd_device_set_values(dev.h, ptr, nz + 1, dev.VALUES_NOCHECK, None) == -4
    assert L.cholamd_device_set_values(dev.h, None, nz, 0, None) == -4
    assert L.cholamd_device_set_values(dev.h, ptr, nz, -1, None) == -4
    assert L.cholamd_device_set_values(dev.h, ptr, nz, 2, None) == -4
    assert np.array_equal(bits(filled(dev)), bits(before))       # nothing written
    assert L.cholamd_device_set_values(dev.h, ptr, nz, 0, None) == 0
    assert np.array_equal(bits(filled(dev)), bits(filled(ca.Device(S2.plan, 0))))
