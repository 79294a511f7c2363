"""GPU factor, solves and queries on synthetic elimination trees (tests/tree_inputs.py): a separator of every size around every kernel's size
threshold as a leaf, as a middle separator and as the root, under CHOLAMD_POISON=1 with guarded caller buffers.

The kernels choose their code path by separator size (tile 16, one-wave TRSM 64, selected-inversion blocks and Schur pieces 64, fp32 LDS pivot 128,
pivot split and throughput TRSM 144, followers 160, program-launch split 176, fused POTRF+TRSM 192, span inverses 256, register-resident POTRF 272),
and where a grid puts a separator near one of them, it does not choose its place in the tree.  Printed by a one-off script from plan.sep_sizes:

  separator sizes the suite had: the four fixtures, spd_inputs' inputs before the trees and every generated grid of the GPU files (20 grids from
  3 x 3 x 1 to 100^3), places in the tree as they fall -- up to 600 columns:
    2 3 4 5 6 7 8 9 10 14 15 16 17 18 19 20 22 23 24 25 26 30 33 34 35 36 39 51 56 59 60 64 70 72 81 86 90 97 98 100 101 102 115 121 125 128 132 140
    143 144 150 161 162 163 171 174 177 180 190 196 200 201 206 210 216 218 225 236 253 259 264 288 300 324 360 361 380 392 400 406 420 435 448 450
    490 510 512 529 540 576 600, and 54 sizes from 605 to 10000
    (within one column of a threshold: 15 16 17 64 128 143 144 161 177 -- nothing at 65, 127, 129, 145, 159, 160, 175, 176, 191 .. 193, 255 .. 257,
    271 .. 273)
  separator sizes of this file (the sweep, each at a leaf, in the middle and at the root, and the named trees):
    1 2 3 5 7 15 16 17 21 29 31 33 37 63 64 65 127 128 129 143 144 145 159 160 161 175 176 177 191 192 193 255 256 257 271 272 273 287 288 289 300
    511 512 513

Measures and tolerances are spd_inputs' (tol_* as functions of u, the longest row k and the equilibrated kappa); the half solves, the logdet and the
selected inversion are held to the bounds of test_gpu_factor_query and test_gpu_selinv.  tests/test_tree_inputs.py shows on the CPU that one dropped
16 x 16 contribution fails these measures."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tree_inputs as ti  # noqa: E402
from guarded import Guarded  # noqa: E402
from spd_inputs import U32, U64  # noqa: E402
from test_gpu_factor import LAUNCH_PATHS  # noqa: E402
from test_gpu_factor_query import BWD, FWD, half_ref, logdet_tol, rel_cols  # noqa: E402
from test_gpu_general_spd import MAX_ITER, PIVOT_PATHS, _dense, _diag_index, _ids  # noqa: E402
from test_gpu_general_spd import _factor as plain_factor, _solve as plain_solve  # noqa: E402
from test_gpu_poison import _block, _factor, _solve  # noqa: E402
from test_gpu_selinv import _check_all  # noqa: E402

FACTOR_PATHS = [{}, {"program": 0}, {"program": 0, "fuse": 0}, {"program": 0, "trsm_wt_min": 1}, {"skyline": 0}, "f32"]
SWEEP = [(pos, leaf) for pos, leaf in (("leaf", "dense"), ("leaf", ("band", 17)), ("middle", "dense"), ("root", "dense"))]
SWEEP_IDS = ["leaf_dense", "leaf_band17", "middle", "root"]


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("CHOLAMD_POISON", "1")
    for v in ("CHOLAMD_SOLVE_NO_BAND", "CHOLAMD_SOLVE_NO_INV256", "CHOLAMD_SOLVE_REFERENCE_SHAPE"):
        monkeypatch.delenv(v, raising=False)


@pytest.fixture(scope="module")
def spd(tmp_path_factory):
    return lambda name: ti.cached(tmp_path_factory, name)


def _device(plan, path):
    import cholesky_amd as ca
    dev = ca.Device(plan, 0)
    for k, v in ({} if path == "f32" else path).items():
        dev.set_option(k, v)
    return dev


def _check_factor(S, a, f32, what):
    u = U32 if f32 else U64
    L = _dense(S, a.t)
    if not f32:
        assert np.array_equal(L != 0, S.Lo != 0), what                # the oracle's zero pattern, entry for entry
    assert S.row_error(L) <= S.tol_factor(u), what                    # vs dense numpy
    assert S.row_error(L, S.Lo) <= S.tol_factor(u), what              # vs the CPU oracle
    assert S.reconstruction(L) <= S.tol_reconstruction(u), what


def _block_refs(S, k, seed=7):
    """k right-hand sides (the first is the input's own) and their reference solutions: the dense fp64 factor and one correction."""
    import scipy.linalg as sl
    rng = np.random.default_rng(seed)
    B = S.s[:, None] * rng.standard_normal((S.n, k))
    B[:, 0] = S.rhs
    p = S.perm
    X = sl.cho_solve((S.Ld, True), B[p])
    X += sl.cho_solve((S.Ld, True), B[p] - S.PAP @ X)
    Xref = np.empty_like(X)
    Xref[p] = X
    return B, Xref


def _check_solves(S, dev, a, B, Xref, u=U64, what=""):
    """solve and solve_nrhs with 1 and 33 columns on guarded buffers with padding rows."""
    x, _ = _solve(dev, a, S.rhs, "fp32" if u == U32 else "fp64")
    if u == U64:
        assert S.backward_error(x, S.rhs) <= S.tol_backward(), what
    assert S.forward_error(x) <= S.tol_forward(u), what
    for k in (1, 33):
        Bg, Xg = _block(B[:, :k], S.n + 3), Guarded(S.n, k, S.n + 3)
        snap = Bg.snapshot()
        dev.solve_nrhs(a.t, Bg.t, Xg.t)
        dev.sync()
        Bg.assert_unchanged(snap, f"B, nrhs {k}")
        Xg.assert_guards(f"X, nrhs {k}")
        X = Xg.numpy()
        for j in range(k):
            assert S.forward_error(X[:, j], Xref[:, j]) <= S.tol_forward(u), (what, k, j)


def _check_queries(S, dev, a, B, name):
    """Half solves, logdet and the selected inversion of an fp64 factor against the dense references."""
    tol = S.tol_forward()
    Yref = half_ref(S.Ld, S.perm, B[:, :1], FWD)
    Xref = half_ref(S.Ld, S.perm, Yref, BWD)
    for which, v, ref in ((FWD, B[:, 0], Yref), (BWD, Yref[:, 0], Xref)):
        b, x = Guarded(S.n, values=v), Guarded(S.n)
        snap = b.snapshot()
        dev.solve_half(a.t, b.t, x.t, which)
        dev.sync()
        b.assert_unchanged(snap, "half solve b")
        x.assert_guards("half solve x")
        got = x.numpy()
        e = rel_cols(got[:, None], ref).max() if which == FWD else S.forward_error(got, ref[:, 0])
        assert e <= tol, (name, which, e, tol)
    ld = dev.logdet(a.t)
    ref = 2.0 * float(np.sum(np.log(np.diag(S.Ld))))
    assert abs(ld - ref) <= logdet_tol(S.k, S.kappa, S.n, U64), (name, ld, ref)
    snap = a.snapshot()
    z, d, v = Guarded(S.plan.arena_doubles), Guarded(S.n), Guarded(S.plan.nz)
    dev.selinv(a.t, z.t)
    dev.selinv_diag(z.t, out=d.t)
    dev.selinv_entries(z.t, out=v.t)
    dev.sync()
    a.assert_unchanged(snap, "arena")
    for g, what in ((z, "Z arena"), (d, "diag"), (v, "entries")):
        g.assert_guards(what)
    _check_all(S, dev, z.t, name, diag=d.t, vals=v.t)


def _check_refinement(S, dev, a32, what=""):
    tol = 1e-12
    x, (it, rel) = _solve(dev, a32, S.rhs, "refine", max_iter=MAX_ITER, tol=tol)
    assert rel <= tol and it <= S.refine_iterations(tol), (what, it, rel, S.refine_iterations(tol))
    true = S.true_relres(x, S.rhs)
    assert abs(rel - true) <= 1e-13 + 0.5 * true, what               # the residual it reports is the true one
    assert S.forward_error(x) <= S.tol_forward(), what


# ------------------------------------------------------------------------------------------------
# a. the threshold sweep
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", ti.SWEEP_SIZES)
@pytest.mark.parametrize("position,leaf", SWEEP, ids=SWEEP_IDS)
def test_threshold_sweep(position, leaf, s, tmp_path, monkeypatch):
    S = ti.sweep(tmp_path, position, s, leaf)
    P = S.plan
    heap = {"leaf": 4, "middle": 2, "root": 1}[position]
    assert P.sep_sizes[P.tree[heap - 1] - 1] == s and P.levels == 3
    name = f"{position} {leaf} {s}"
    kept = {}
    for path in FACTOR_PATHS:
        f32 = path == "f32"
        dev = _device(P, path)
        a = _factor(dev, f32)                                          # guarded arena; info == (0, 0); guards intact
        _check_factor(S, a, f32, (name, path))
        if f32 or path == {}:
            kept[f32] = (dev, a)
    B, Xref = _block_refs(S, 33)
    dev, a = kept[False]
    _check_solves(S, dev, a, B, Xref, what=name)
    _check_queries(S, dev, a, B, name)
    if s >= 255:
        monkeypatch.setenv("CHOLAMD_SOLVE_NO_INV256", "1")            # read when a device object builds its solve lists (first solve)
        dev2 = _device(P, {})
        _check_solves(S, dev2, _factor(dev2), B, Xref, what=name + " no inv256")
        monkeypatch.delenv("CHOLAMD_SOLVE_NO_INV256")
    dev32, a32 = kept[True]
    _check_solves(S, dev32, a32, B, Xref, u=U32, what=name + " fp32")
    _check_refinement(S, dev32, a32, name)


# ------------------------------------------------------------------------------------------------
# b. every launch path on the named trees
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", LAUNCH_PATHS, ids=_ids)
@pytest.mark.parametrize("name", ["tree_over", "tree_skew"])
def test_every_launch_path_on_trees(name, opts, spd):
    S = spd(name)
    dev, arena = plain_factor(S, opts)
    assert dev.info() == (0, 0)
    L = _dense(S, arena)
    assert np.array_equal(L != 0, S.Lo != 0)
    assert S.row_error(L) <= S.tol_factor()
    x = plain_solve(dev, arena, S.rhs)
    assert S.forward_error(x) <= S.tol_forward()


# ------------------------------------------------------------------------------------------------
# c. pivot failure at the thresholds
# ------------------------------------------------------------------------------------------------
PIVOT_SEPS = [(3, 145), (2, 177), (1, 193), (4, 257), (5, 273)]       # (heap index, columns) in tree_over
SPLIT_NB, RR_MAXN = 144, 272                                           # CHOL_SPLIT_NB, CHOL_RR_MAXN
SPLIT_MINS = {"levels": 144, "program": 176}                           # CHOL_SPLIT_MIN; CHOL_PROG_SPLIT_MIN, the program launch's at the default split


def pivot_blocking(n, split_min):
    """(blocks, block width) of a pivot of n columns as chol_schedule.c cuts it (pivot_blocks, pivot_block_width): wider than split_min, equal
    blocks of at most CHOL_SPLIT_NB columns, the width rounded up to a multiple of 16; block st starts at column st * width."""
    nb = -(-n // SPLIT_NB) if n > split_min or n > RR_MAXN else 1
    return nb, n if nb == 1 else (-(-n // nb) + 15) // 16 * 16


def last_block_start(n, split_min):
    """First column of the last column block: 0 where the pivot is not split."""
    nb, bw = pivot_blocking(n, split_min)
    c = (nb - 1) * bw
    assert (c == 0 and nb == 1) or (0 < c < n and c % bw == 0 and bw % 16 == 0 and n - c <= bw <= SPLIT_NB)
    return c


# level by level 145 = 80 + 65, 177 = 96 + 81, 193 = 112 + 81, 257 = 144 + 113, 273 = 144 + 129; the program launch keeps 145 whole (column 0)
PIVOT_EDGES = {m: sorted({last_block_start(m, sm) for sm in SPLIT_MINS.values()}) for _, m in PIVOT_SEPS}
assert PIVOT_EDGES == {145: [0, 80], 177: [96], 193: [112], 257: [144], 273: [144]}
PIVOT_CASES = [(h, m, c) for h, m in PIVOT_SEPS for c in PIVOT_EDGES[m] + [m - 1]]


@pytest.mark.parametrize("heap,size,col", PIVOT_CASES)
def test_pivot_failure_at_the_thresholds(heap, size, col, spd):
    """A'_kk = A_kk - 1.5 L_kk^2 (test_gpu_general_spd's construction) at the first column of the last column block at the default split and at
    the last column of the separators of 145, 177, 193, 257 and 273 columns.  The block edge is the library's own: equal blocks rounded up to 16
    columns, for the level schedule's split (wider than 144) and for the program launch's (wider than 176, so 145 is whole there: column 0);
    every path gets every column.  info = (k - offset + 1, separator), cross-checked with LAPACK dpotrf; afterwards the same device object
    factors good values to (0, 0)."""
    import torch
    from scipy.linalg import lapack
    S = spd("tree_over")
    P = S.plan
    lbl = int(P.tree[heap - 1])
    off = int(P.sep_offsets[lbl - 1])
    assert P.sep_sizes[lbl - 1] == size and 0 <= col < size
    k = off + col
    host = P.fill_host()
    newv = S.PAP[k, k] - 1.5 * S.Ld[k, k] ** 2
    host[_diag_index(P, host, k)] = newv
    Ap = S.PAP.copy()
    Ap[k, k] = newv
    assert lapack.dpotrf(Ap, lower=1)[1] == k + 1
    expect = (col + 1, lbl)
    for path in PIVOT_PATHS:
        f32 = path == "f32"
        dev = _device(P, path)
        bad = Guarded(P.arena_doubles, dtype=torch.float32 if f32 else torch.float64, values=host)
        (dev.factor_f32 if f32 else dev.factor)(bad.t)
        dev.sync()
        assert dev.info() == expect, (path, dev.info(), expect)
        bad.assert_guards("arena of the failed factorisation")
        _factor(dev, f32)                                              # info == (0, 0)


# ------------------------------------------------------------------------------------------------
# d. one-level and two-level trees
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ti.SINGLE)
def test_shallow_trees(name, spd):
    import cholesky_amd as ca
    S = spd(name)
    P = S.plan
    assert P.levels == {"tree_single": 1, "tree_two": 2}[name]
    B, Xref = _block_refs(S, 33)
    for path in ({}, {"program": 0}, "f32"):
        f32 = path == "f32"
        dev = _device(P, path)
        a = _factor(dev, f32)
        _check_factor(S, a, f32, (name, path))
        _check_solves(S, dev, a, B, Xref, u=U32 if f32 else U64, what=(name, path))
        if f32:
            _check_refinement(S, dev, a, name)
        elif path == {}:
            _check_queries(S, dev, a, B, name)
    dev = _device(P, {})
    if P.levels == 1:                                                  # nothing below the root to eliminate: refused
        with pytest.raises(ca.CholamdError, match="kept levels"):
            P.schur_size(1)
        return
    arena = Guarded(P.arena_doubles)
    dev.fill(arena.t)
    dev.schur_factor(arena.t, 1)
    dev.sync()
    assert dev.info() == (0, 0)
    arena.assert_guards("arena")
    m = P.schur_size(1)
    t0 = S.n - m
    A = S.PAP
    S1 = A[t0:, t0:] - A[:t0, t0:].T @ np.linalg.solve(A[:t0, :t0], A[:t0, t0:])       # the two CPU routes and the gate of test_gpu_schur
    S2 = A[t0:, t0:] - S.Ld[t0:, :t0] @ S.Ld[t0:, :t0].T
    scale = float(np.abs(S1).max())
    gate = max(1e-12, 100.0 * float(np.abs(S1 - S2).max()) / scale)
    got = dev.schur(arena.t, 1).cpu().numpy()
    err = max(float(np.abs(got - S1).max()), float(np.abs(got - S2).max())) / scale
    print(f"schur {name} k = 1: m = {m}, gate {gate:.3g}, error {err:.3g}")
    assert np.isfinite(got).all() and err <= gate
    assert np.array_equal(got, got.T)
    assert np.array_equal(got, P.schur_host(1, arena.numpy()))
