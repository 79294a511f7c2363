"""GPU factor, solves, pivot failure and sharding on general SPD inputs (tests/spd_inputs.py): mixed-sign random values on the fixtures' own
patterns, 27-point / 9-point / random-subset stencils on generated grids, a symmetric diagonal scaling over six decades, an ill-conditioned
input and a matrix outside fp32's range.  Every other GPU test factors a grid Laplacian (an M-matrix of nearly equal values), where a lost
sign of an update product or a swapped value of A does not change the factor.  Measures and tolerances: spd_inputs' docstring."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import spd_inputs as si  # noqa: E402
from sharded import assemble as _assemble  # noqa: E402
from spd_inputs import U32  # noqa: E402
from test_gpu_factor import LAUNCH_PATHS  # noqa: E402

MAX_ITER = 30


def _ids(o):
    return "+".join(f"{k}={v}" for k, v in o.items()) or "default"


@pytest.fixture(scope="module")
def spd(tmp_path_factory):
    return lambda name: si.cached(tmp_path_factory, name)


def _factor(S, opts=None, f32=False):
    import cholesky_amd as ca
    dev = ca.Device(S.plan, 0)
    for k, v in (opts or {}).items():
        dev.set_option(k, v)
    if f32:
        a = dev.new_arena_f32()
        dev.fill_f32(a)
        dev.factor_f32(a)
    else:
        a = dev.new_arena()
        dev.fill(a)
        dev.factor(a)
    dev.sync()
    return dev, a


def _dense(S, arena):
    return np.tril(S.plan.arena_to_dense(arena.cpu().numpy().astype(np.float64)))


def _solve(dev, arena, b, f32=False):
    import torch
    d_b = torch.from_numpy(b).cuda()
    d_x = torch.empty_like(d_b)
    (dev.solve_f32 if f32 else dev.solve)(arena, d_b, d_x)
    dev.sync()
    return d_x.cpu().numpy()


# ------------------------------------------------------------------------------------------------
# a. fp64 factor parity
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", si.NAMES)
def test_fp64_factor_and_solve_match_dense_references(name, spd):
    S = spd(name)
    dev, arena = _factor(S)
    assert dev.info() == (0, 0)
    L = _dense(S, arena)
    assert np.array_equal(L != 0, S.Lo != 0)                       # the oracle's zero pattern, entry for entry
    assert S.row_error(L) <= S.tol_factor()                        # vs dense numpy
    assert S.row_error(L, S.Lo) <= S.tol_factor()                  # vs the CPU oracle
    assert S.reconstruction(L) <= S.tol_reconstruction()
    x = _solve(dev, arena, S.rhs)
    assert S.backward_error(x, S.rhs) <= S.tol_backward()
    assert S.forward_error(x) <= S.tol_forward()


# ------------------------------------------------------------------------------------------------
# b. every launch path, the level-schedule variants
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", LAUNCH_PATHS, ids=_ids)
def test_every_launch_path_on_random_values(opts, spd):
    """test_alternative_launch_paths_keep_parity's option list on lapl_3375 with mixed-sign random values."""
    S = spd("lapl_3375x3375")
    dev, arena = _factor(S, opts)
    assert dev.info() == (0, 0)
    L = _dense(S, arena)
    assert np.array_equal(L != 0, S.Lo != 0)
    assert S.row_error(L) <= S.tol_factor()
    x = _solve(dev, arena, S.rhs)
    assert S.forward_error(x) <= S.tol_forward()


LEVEL_VARIANTS = [
    {"program": 0, "trsm_wt_min": 1},
    {"split_min": 64, "split_nb": 64, "super_blocks": 1},
    {"split_min": 64, "split_nb": 64, "super_blocks": 2},
    {"split_min": 64, "split_nb": 64, "super_blocks": 4},
    {"program": 0, "mt_min_tiles": 1, "merge_targets": 0},
    {"program": 0, "mt_min_tiles": 1, "merge_targets": 1},
]


@pytest.mark.parametrize("name", ["g18_full", "g16_subset"])
def test_level_schedule_variants_on_general_patterns(name, spd):
    S = spd(name)
    for opts in LEVEL_VARIANTS:
        dev, arena = _factor(S, opts)
        assert dev.info() == (0, 0), opts
        L = _dense(S, arena)
        assert S.row_error(L) <= S.tol_factor(), opts
        assert np.array_equal(L != 0, S.Lo != 0), opts
    for f32 in (False, True):
        res = []
        for env in (0, 1):
            dev, arena = _factor(S, {"program": 0, "mt_min_tiles": 1, "leaf_envelope": env}, f32=f32)
            assert dev.info() == (0, 0)
            res.append(arena.cpu().numpy().astype(np.float64))
        assert np.array_equal(res[0] == 0.0, res[1] == 0.0)          # the envelope skips only what is zero
        L = _dense(S, arena)
        assert S.row_error(L) <= S.tol_factor(U32 if f32 else si.U64)


# ------------------------------------------------------------------------------------------------
# c. solves
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lapl_3375_scaled", "g12_full", "g16_subset", "g20_2d"])
def test_solves_on_general_inputs(name, spd, monkeypatch):
    import torch
    import cholesky_amd as ca
    S = spd(name)
    n = S.n
    rng = np.random.default_rng(7)
    B = S.s[:, None] * rng.standard_normal((n, 33))
    B[:, 0] = S.rhs
    Xref = np.stack([S.reference_solve(B[:, j]) for j in range(33)], axis=1)
    xs = {}
    for no_band in (False, True):
        # the device object builds its solve lists at its first solve and reads CHOLAMD_SOLVE_NO_BAND (present or not) then: the variable stays
        # as it is for the leg's whole device
        if no_band:
            monkeypatch.setenv("CHOLAMD_SOLVE_NO_BAND", "1")
        else:
            monkeypatch.delenv("CHOLAMD_SOLVE_NO_BAND", raising=False)
        dev, arena = _factor(S)
        assert dev.info() == (0, 0)
        x = _solve(dev, arena, S.rhs)
        assert S.backward_error(x, S.rhs) <= S.tol_backward()
        assert S.forward_error(x) <= S.tol_forward()
        xs[no_band] = x
        for k in (1, 33):
            dB = torch.from_numpy(np.ascontiguousarray(B[:, :k].T)).cuda().T
            dX = torch.empty(k, n, dtype=torch.float64, device="cuda").T
            dev.solve_nrhs(arena, dB, dX)
            dev.sync()
            X = dX.cpu().numpy()
            for j in range(k):
                assert S.forward_error(X[:, j], Xref[:, j]) <= S.tol_forward(), (k, j)
        seps, runs = S.plan.solve_skips(S.plan.levels - 1)   # the same list builder, the same environment: this leg's solve lists skip or not
        assert bool(seps[:, 2].any() or runs[:, 4].any()) != no_band
        del dev, arena
    monkeypatch.delenv("CHOLAMD_SOLVE_NO_BAND", raising=False)
    assert S.forward_error(xs[False], xs[True]) <= S.tol_forward()        # banded and full solve lists: the same x
    # the fp32 factor: one solve to fp32 accuracy, refinement to fp64
    dev = ca.Device(S.plan, 0)
    a32 = dev.new_arena_f32()
    dev.fill_f32(a32)
    dev.factor_f32(a32)
    dev.sync()
    assert dev.info() == (0, 0)
    x = _solve(dev, a32, S.rhs, f32=True)
    assert S.forward_error(x) <= S.tol_forward(U32)
    dB = torch.from_numpy(np.ascontiguousarray(B.T)).cuda().T
    dX = torch.empty(33, n, dtype=torch.float64, device="cuda").T
    tol = 1e-12
    it, rel = dev.solve_refine_nrhs(a32, dB, dX, max_iter=MAX_ITER, tol=tol)
    X = dX.cpu().numpy()
    for j in range(33):
        true = S.true_relres(X[:, j], B[:, j])
        assert abs(rel[j] - true) <= 1e-13 + 0.5 * true   # the residual it reports is the true one
    assert (rel <= tol).all() and it <= S.refine_iterations(tol), (it, rel.max())
    for j in range(33):
        assert S.forward_error(X[:, j], Xref[:, j]) <= S.tol_forward(), j


# ------------------------------------------------------------------------------------------------
# d. fp32 factor and refinement, an input beyond fp32
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lapl_3375x3375", "lapl_3375_scaled", "g12_full", "g16_subset", "g18_full", "g7_ragged"])
def test_fp32_factor_and_refinement(name, spd):
    import torch
    S = spd(name)
    dev, a32 = _factor(S, f32=True)
    assert dev.info() == (0, 0)
    L = _dense(S, a32)
    assert S.row_error(L) <= S.tol_factor(U32)
    d_b = torch.from_numpy(S.rhs).cuda()
    d_x = torch.empty_like(d_b)
    tol = 1e-12
    it, rel = dev.solve_refine(a32, d_b, d_x, max_iter=MAX_ITER, tol=tol)
    x = d_x.cpu().numpy()
    assert rel <= tol and it <= S.refine_iterations(tol), (it, rel, S.refine_iterations(tol))
    true = S.true_relres(x, S.rhs)
    assert abs(rel - true) <= 1e-13 + 0.5 * true
    assert S.forward_error(x) <= S.tol_forward()


def test_refinement_never_claims_convergence_it_did_not_reach(tmp_path):
    """kappa ~ 1e9 (negative-sign 27-point stencil + 1e-7 I): beyond what an fp32 factor refines.  The library may report a failed fp32 pivot, a
    residual above tol that is the true one, or the documented NaN error -- never rel <= tol with a wrong x."""
    import torch
    import cholesky_amd as ca
    S = si.SPD(tmp_path, (12, 12, 12, 4, 16), 5, pattern="full", signs="negative", sigma=1e-7, name="illcond")
    assert S.kappa > 1e8
    dev, a32 = _factor(S, f32=True)
    info = dev.info()
    if info[0] > 0:
        return
    d_b = torch.from_numpy(S.rhs).cuda()
    d_x = torch.empty_like(d_b)
    tol = 1e-13
    try:
        it, rel = dev.solve_refine(a32, d_b, d_x, max_iter=MAX_ITER, tol=tol)
    except ca.CholamdError as e:
        assert "nan" in str(e).lower(), e
        return
    x = d_x.cpu().numpy()
    true = S.true_relres(x, S.rhs)
    assert abs(rel - true) <= 1e-13 + 0.5 * true
    if rel <= tol:
        assert S.forward_error(x) <= S.tol_forward()


# ------------------------------------------------------------------------------------------------
# e. pivot failure anywhere
# ------------------------------------------------------------------------------------------------
def _position(S, where):
    P = S.plan
    lv = P.levels
    leaf = lambda lbl: S.level_of(lbl) == lv - 1  # noqa: E731
    labels = range(1, P.nsep + 1)
    if where in ("leaf_tile_first", "leaf_tile_last"):
        lbl = next(lb for lb in labels if leaf(lb) and P.sep_sizes[lb - 1] >= 48)
        return int(P.sep_offsets[lbl - 1]) + (16 if where == "leaf_tile_first" else 31)
    if where == "banded_leaf":
        seps, _ = P.solve_skips(lv - 1)
        off, n, band = next(s for s in seps if 0 < s[2] <= 64)
        return int(off) + int(n) - 20
    if where == "middle":   # A'_kk stays positive: only the descendants' updates make the pivot fail
        ratio = np.diag(S.Ld) ** 2 / np.diag(S.PAP)
        cand = [k for lb in labels if 0 < S.level_of(lb) < lv - 1
                for k in range(int(P.sep_offsets[lb - 1]), int(P.sep_offsets[lb - 1] + P.sep_sizes[lb - 1])) if ratio[k] < 0.6]
        return cand[len(cand) // 2]
    root = P.nsep
    off, size = int(P.sep_offsets[root - 1]), int(P.sep_sizes[root - 1])
    assert size == 324
    return off + (300 if where == "root_block2" else size - 1)


PIVOT_CASES = [("g12_full", "leaf_tile_first"), ("g12_full", "leaf_tile_last"), ("g12_full", "banded_leaf"), ("g12_full", "middle"),
               ("g18_full", "middle"), ("g18_full", "root_block2"), ("g18_full", "root_last")]
PIVOT_PATHS = [{}, {"program": 0}, {"program": 0, "fuse": 0}, "f32"]


@pytest.mark.parametrize("name,where", PIVOT_CASES)
def test_pivot_failure_anywhere_reports_its_column(name, where, spd):
    """A'_kk = A_kk - 1.5 L_kk^2: columns before k are unchanged, pivot k is the first that fails ((L'_kk)^2 = -0.5 L_kk^2); expected info =
    (k - offset(sep) + 1, sep), cross-checked with LAPACK dpotrf on the dense P A' P^T.  After each failure the same device object factors
    good values to (0, 0)."""
    import torch
    import cholesky_amd as ca
    from scipy.linalg import lapack
    S = spd(name)
    P = S.plan
    k = _position(S, where)
    host = P.fill_host()
    newv = S.PAP[k, k] - 1.5 * S.Ld[k, k] ** 2
    if where == "middle":
        assert newv > 0
    idx = _diag_index(P, host, k)
    host[idx] = newv
    Ap = S.PAP.copy()
    Ap[k, k] = newv
    assert lapack.dpotrf(Ap, lower=1)[1] == k + 1
    lbl, off = S.sep_of(k)
    expect = (k - off + 1, lbl)
    for path in PIVOT_PATHS:
        dev = ca.Device(P, 0)
        f32 = path == "f32"
        for key, v in ({} if f32 else path).items():
            dev.set_option(key, v)
        bad = torch.from_numpy(host.astype(np.float32) if f32 else host).cuda()
        (dev.factor_f32 if f32 else dev.factor)(bad)
        dev.sync()
        assert dev.info() == expect, (path, dev.info(), expect)
        good = dev.new_arena_f32() if f32 else dev.new_arena()
        (dev.fill_f32 if f32 else dev.fill)(good)
        (dev.factor_f32 if f32 else dev.factor)(good)
        dev.sync()
        assert dev.info() == (0, 0), path


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


def test_nan_in_a_leaf_entry_is_a_failed_pivot(spd):
    """A NaN in one off-diagonal entry (i, j) of a leaf: L_ij is NaN, so is the pivot of row i, and no pivot before it (rows between j and i do not
    involve row i): info = (i + 1, leaf), never (0, 0).  (LAPACK's dpotrf is no cross-check here: the OpenBLAS one scipy bundles tests
    ajj <= 0 only and passes a NaN pivot.)"""
    import torch
    import cholesky_amd as ca
    S = spd("g12_full")
    P = S.plan
    host = P.fill_host()
    lbl = next(lb for lb in range(1, P.nsep + 1) if S.level_of(lb) == P.levels - 1)
    off, n = int(P.sep_offsets[lbl - 1]), int(P.sep_sizes[lbl - 1])
    D = S.PAP[off:off + n, off:off + n]
    i, j = [(a, b) for a, b in zip(*np.nonzero(np.tril(D, -1))) if a >= 20][0]
    b = P.blocks[(P.blocks[:, 0] == lbl) & (P.blocks[:, 1] == lbl)][0]
    idx = int(b[7]) + int(i) + int(j) * int(b[6])
    probe = np.zeros_like(host)
    probe[idx] = 1.0
    assert P.arena_to_dense(probe)[off + i, off + j] == 1.0
    host[idx] = np.nan
    for path in PIVOT_PATHS:
        dev = ca.Device(P, 0)
        f32 = path == "f32"
        for key, v in ({} if f32 else path).items():
            dev.set_option(key, v)
        bad = torch.from_numpy(host.astype(np.float32) if f32 else host).cuda()
        (dev.factor_f32 if f32 else dev.factor)(bad)
        dev.sync()
        assert dev.info() == (i + 1, lbl), (path, dev.info())


# ------------------------------------------------------------------------------------------------
# f. sharded
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("name", ["g16_subset", "tree_skew"])
def test_sharded_factor_of_a_general_input(name, world, f32, spd):
    """g16_subset: a grid's balanced subtrees; tree_skew: subtrees of very unequal weight (leaves of 1 and of 289 columns)."""
    import cholesky_amd as ca
    from cholesky_amd import parallel
    from cholesky_amd.device import factor_multi
    S = spd(name)
    plan = S.plan
    _, ref_t = _factor(S, f32=f32)
    ref = ref_t.cpu().numpy().astype(np.float64)
    tail = parallel.tail_offset(plan, world)
    devs, arenas = [], []
    for r in range(world):
        dev = ca.Device(plan, 0)
        dev.set_partition(r, world)
        a = dev.new_arena_f32() if f32 else dev.new_arena()
        (dev.fill_f32 if f32 else dev.fill)(a)
        devs.append(dev)
        arenas.append(a)
    factor_multi(devs, arenas, local=True)
    for dev in devs:
        assert dev.info() == (0, 0)
    parts = [a.cpu().numpy().astype(np.float64) for a in arenas]
    for r in range(1, world):
        assert np.array_equal(parts[r][tail:], parts[0][tail:])
    out = _assemble(plan, parts, world)
    L = np.tril(plan.arena_to_dense(out))
    u = U32 if f32 else si.U64
    assert S.row_error(L, np.tril(plan.arena_to_dense(ref))) <= S.tol_factor(u)
    assert S.row_error(L) <= S.tol_factor(u)


# ------------------------------------------------------------------------------------------------
# g. fp32 range
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decades", [40.0, -42.0])
def test_fp32_refuses_a_matrix_outside_its_range(decades, tmp_path):
    """D A D with D_ii = 10^(decades / 2) on a random third of the unknowns: entries beyond FLT_MAX (10^40 A) or a diagonal below FLT_MIN
    (10^-42 A).  The fp32 fill and factor refuse with an argument error; the fp64 path factors the matrix as usual."""
    import cholesky_amd as ca
    S = si.SPD(tmp_path, (7, 5, 3, 3, 4), 3, pattern="full", oracle=False, name="range")
    rng = np.random.default_rng(11)
    d = np.where(rng.random(S.n) < 0.3, 10.0 ** (decades / 2), 1.0)
    val = S.val * d[S.row] * d[S.col]
    si.write_mtx(S.mtx, S.n, S.row, S.col, val)
    plan = ca.Plan(S.mtx, S.ord, S.clust)
    dev = ca.Device(plan, 0)
    a32 = dev.new_arena_f32()
    with pytest.raises(ca.CholamdError, match="range"):
        dev.fill_f32(a32)
    with pytest.raises(ca.CholamdError, match="range"):
        dev.factor_f32(a32)
    a = dev.new_arena()
    dev.fill(a)
    dev.factor(a)
    dev.sync()
    assert dev.info() == (0, 0)
    L = np.tril(plan.arena_to_dense(a.cpu().numpy()))
    Ad = plan.arena_to_dense(plan.fill_host())
    Ad = Ad + np.tril(Ad, -1).T
    s = np.sqrt(np.diag(Ad))
    assert np.abs((L @ L.T - Ad) / s[:, None] / s[None, :]).max() <= 1e-13


# ------------------------------------------------------------------------------------------------
# h. leaves wider than 4096 columns
# ------------------------------------------------------------------------------------------------
def test_leaf_wider_than_4096_columns(tmp_path):
    """Problem(20, 20, 25, 2, 64): two leaves of 4800 columns (300 tiles: a tile index above 255 in the leaf skylines).  Factor checked on
    random probes, ||L (L^T v) - P A P^T v|| / (||A|| ||v||), and a solve's componentwise backward error, both against the sparse A."""
    import scipy.sparse as sp
    S = si.SPD(tmp_path, (20, 20, 25, 2, 64), 21, pattern="own", oracle=False, dense=False, name="wide")
    P = S.plan
    assert max(P.sep_sizes) == 4800
    dev, arena = _factor(S)
    assert dev.info() == (0, 0)
    L = si.arena_to_sparse(P, arena.cpu().numpy())    # no dense n x n copy (n = 10 000)
    A = S.A_sparse
    PAP = S.permuted_sparse()
    rng = np.random.default_rng(3)
    k = int(np.diff(L.indptr).max())
    for _ in range(3):
        v = rng.standard_normal(S.n)
        err = np.linalg.norm(L @ (L.T @ v) - PAP @ v) / (sp.linalg.norm(PAP) * np.linalg.norm(v))
        assert err <= si.C_REC * (k + 1) * si.U64 * np.sqrt(S.n)
    b = rng.standard_normal(S.n)
    x = _solve(dev, arena, b)
    r = np.abs(b - A @ x)
    be = (r / (abs(A) @ np.abs(x) + np.abs(b))).max()
    assert be <= si.C_BE * (k + 1) * si.U64
