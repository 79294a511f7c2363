"""The GPU paths on poisoned scratch and guarded caller buffers.

Every test sets CHOLAMD_POISON=1 before it creates its device objects: every floating-point buffer the library allocates (work arenas, solve
and refinement vectors, block-solve chunks, span inverses, exchange staging, rank arenas) then starts as NaN and has a guard tail.  A kernel
that reads a value it does not own -- even to multiply it by zero or to drop it in a row that is never stored -- turns a result into NaN here,
where the allocator's usual zeros or finite leftovers would hide it.  Every arena, b, x, B and X is a `guarded.Guarded` view: NaN guards
around it (and NaN padding rows in B and X) that must keep their bits, and inputs that must not change at all.

Tolerances are those of the tests each part mirrors: test_gpu_factor (fixtures), test_gpu_generated and test_gpu_mixed (oracle solves,
refinement), test_gpu_general_spd (general SPD inputs, spd_inputs' derived bounds), test_distributed (sharded)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import spd_inputs as si  # noqa: E402
from conftest import CASES, case_paths  # noqa: E402
from guarded import Guarded  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from spd_inputs import U32, U64  # noqa: E402
from test_gpu_factor import TOL_L  # noqa: E402
from test_gpu_general_spd import MAX_ITER, _dense, _ids  # noqa: E402

ALL_ONES64 = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("CHOLAMD_POISON", "1")
    for v in ("CHOLAMD_SOLVE_NO_BAND", "CHOLAMD_SOLVE_NO_INV256", "CHOLAMD_SOLVE_REFERENCE_SHAPE"):
        monkeypatch.delenv(v, raising=False)


@pytest.fixture(scope="module")
def spd(tmp_path_factory):
    return lambda name: si.cached(tmp_path_factory, name)


def _arena(dev, f32=False):
    import torch
    return Guarded(dev.plan.arena_doubles, dtype=torch.float32 if f32 else torch.float64)


def _factor(dev, f32=False):
    """Guarded arena, filled and factored on `dev`; info (0, 0) and the guards checked."""
    a = _arena(dev, f32)
    (dev.fill_f32 if f32 else dev.fill)(a.t)
    (dev.factor_f32 if f32 else dev.factor)(a.t)
    dev.sync()
    assert dev.info() == (0, 0)
    a.assert_guards("arena")
    return a


def _solve(dev, a, bvec, kind="fp64", max_iter=20, tol=1e-13):
    """x for b through dev.solve / solve_f32 / solve_refine on guarded b and x (x starts as the NaN pattern); b unchanged, guards intact.
    Returns (x, (iterations, relres) of a refinement or None)."""
    b, x = Guarded(len(bvec), values=bvec), Guarded(len(bvec))
    snap = b.snapshot()
    out = None
    if kind == "refine":
        out = dev.solve_refine(a.t, b.t, x.t, max_iter=max_iter, tol=tol)
    else:
        (dev.solve_f32 if kind == "fp32" else dev.solve)(a.t, b.t, x.t)
    dev.sync()
    b.assert_unchanged(snap, "b")
    x.assert_guards("x")
    return x.numpy(), out


# ------------------------------------------------------------------------------------------------
# a. the switch works
# ------------------------------------------------------------------------------------------------
def test_poison_switch_fills_library_buffers_with_nan():
    import cholesky_amd as ca
    from cholesky_amd import parallel
    plan = ca.Plan(*case_paths("lapl_400x400")[:3])
    dev = ca.Device(plan, 0)
    p = dev.alloc(1000)
    assert (dev.download(p, 1000).view(np.uint64) == ALL_ONES64).all()
    tail = parallel.tail_offset(plan, 2)
    for elem in (8, 4):
        r1 = ca.Device(plan, 0)
        r1.set_partition(1, 2)
        a = r1.alloc_arena(elem)
        assert a.backed_bytes >= 64 << 20         # a rank arena (the scratch chunk + owned ranges), not a plain allocation
        v = a.numpy()
        ones = v.view(np.uint64 if elem == 8 else np.uint32) == (ALL_ONES64 if elem == 8 else np.uint32(0xFFFFFFFF))
        assert ones[tail:].all()      # the shared top: owned by every rank
        assert ones.all()             # the rank's own panels, and the other ranks' (the aliased scratch chunk)
        a.free()


# ------------------------------------------------------------------------------------------------
# b. the reference fixtures, fp64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_fixtures_factor_and_solve_match_golden(case, golden):
    import cholesky_amd as ca
    m, o, c, bf = case_paths(case)
    plan = ca.Plan(m, o, c)
    dev = ca.Device(plan, 0)
    a = _factor(dev)
    g = golden(case)
    L = np.tril(plan.arena_to_dense(a.numpy()))
    assert np.abs(L - g["L"]).max() <= TOL_L
    x, _ = _solve(dev, a, ca.plan.read_vector(bf, plan.n))
    assert np.abs(x - g["x"]).max() <= 1e-10 * max(1.0, np.abs(g["x"]).max())


# ------------------------------------------------------------------------------------------------
# c. ragged spans: the regression test of k_solve_stepw's clamped read past a ragged last span
# ------------------------------------------------------------------------------------------------
SOLVE_CONFIGS = ["default", "CHOLAMD_SOLVE_NO_BAND", "CHOLAMD_SOLVE_NO_INV256", "solve_reference_shape"]


@pytest.fixture(scope="module")
def ragged(tmp_path_factory):
    """{name: (plan files, b, the oracle's x)} of the problems whose root separator ends in a ragged span: two spans (324 = 256 + 68), one span
    (225 = 14 * 16 + 1), three spans (529 = 2 * 256 + 17: the panel of the span before the previous one)."""
    import cholesky_amd as ca
    orc.use_own_kernels()
    out = {}
    prob = ca.Problem(18, 18, 18, 3, 48)
    m, o, c, _ = prob.write(os.path.join(tmp_path_factory.mktemp("ragged"), "gen"))
    out["gen_18_324"] = ((m, o, c), prob.rhs())
    prob = ca.Problem(23, 23, 23, 4, 32)
    m, o, c, _ = prob.write(os.path.join(tmp_path_factory.mktemp("ragged"), "gen"))
    out["gen_23_529"] = ((m, o, c), prob.rhs())
    m, o, c, bf = case_paths("lapl_3375x3375")
    out["lapl_3375_225"] = ((m, o, c), ca.plan.read_vector(bf, 3375))
    res = {}
    for k, (files, b) in out.items():
        O = orc.Oracle(*files)
        O.factor()
        res[k] = (files, b, O.solve(b))
    return res


@pytest.mark.parametrize("config", SOLVE_CONFIGS)
@pytest.mark.parametrize("name,root", [("gen_18_324", 324), ("lapl_3375_225", 225), ("gen_23_529", 529)])
def test_ragged_root_span_solves(name, root, config, ragged, monkeypatch):
    import cholesky_amd as ca
    files, b, xo = ragged[name]
    plan = ca.Plan(*files)
    size = int(plan.sep_sizes[plan.nsep - 1])
    assert size == root and size % 16 != 0
    assert size > 256 or size == 14 * 16 + 1
    if config.startswith("CHOLAMD_"):
        monkeypatch.setenv(config, "1")          # read when the device object builds its solve lists (first solve)
    scale = max(1.0, np.abs(xo).max())
    dev = ca.Device(plan, 0)
    if config == "solve_reference_shape":
        dev.set_option(config, 1)
    a = _factor(dev)
    x, _ = _solve(dev, a, b)
    assert np.abs(x - xo).max() <= 1e-9 * scale
    dev32 = ca.Device(plan, 0)
    if config == "solve_reference_shape":
        dev32.set_option(config, 1)
    a32 = _factor(dev32, f32=True)
    x, _ = _solve(dev32, a32, b, "fp32")
    assert np.isfinite(x).all() and np.abs(x - xo).max() <= 1e-3 * scale      # one fp32-factor solve: single precision
    x, (iters, rel) = _solve(dev32, a32, b, "refine")
    assert rel <= 1e-12 and iters <= 8, (iters, rel)
    assert np.abs(x - xo).max() <= 1e-10 * scale


# ------------------------------------------------------------------------------------------------
# d. general SPD inputs on the launch paths
# ------------------------------------------------------------------------------------------------
POISON_INPUTS = ["g7_ragged", "g16_subset", "g18_full", "g20_2d", "lapl_3375_scaled"]
POISON_PATHS = [
    {},
    {"program": 0},
    {"program": 0, "mt_min_tiles": 1, "merge_targets": 0},
    {"program": 0, "mt_min_tiles": 1, "merge_targets": 1},
    {"leaf_envelope": 0},
    {"split_min": 64, "split_nb": 64, "super_blocks": 2},
    {"program": 0, "trsm_wt_min": 1},
]


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", POISON_INPUTS)
def test_general_inputs_on_launch_paths(name, f32, spd):
    import cholesky_amd as ca
    S = spd(name)
    u = U32 if f32 else U64
    for opts in POISON_PATHS:
        dev = ca.Device(S.plan, 0)
        for k, v in opts.items():
            dev.set_option(k, v)
        a = _factor(dev, f32)
        L = _dense(S, a.t)
        assert S.row_error(L) <= S.tol_factor(u), _ids(opts)
        if f32:
            tol = 1e-12
            x, (it, rel) = _solve(dev, a, S.rhs, "refine", max_iter=MAX_ITER, tol=tol)
            assert rel <= tol and it <= S.refine_iterations(tol), (_ids(opts), it, rel)
        else:
            assert np.array_equal(L != 0, S.Lo != 0), _ids(opts)
            assert S.reconstruction(L) <= S.tol_reconstruction(), _ids(opts)
            x, _ = _solve(dev, a, S.rhs)
            assert S.backward_error(x, S.rhs) <= S.tol_backward(), _ids(opts)
        assert S.forward_error(x) <= S.tol_forward(), _ids(opts)


# ------------------------------------------------------------------------------------------------
# e. block solve: chunk edges, the single-vector fallback, NaN padding, in place, refinement
# ------------------------------------------------------------------------------------------------
NRHS = [1, 3, 4, 5, 6, 7, 31, 32, 33, 35, 36, 38, 65]


@pytest.fixture(scope="module")
def block_ref(spd):
    """g18_full, 65 right-hand sides (the first is the input's own) and their reference solutions (the dense fp64 factor + one correction)."""
    import scipy.linalg as sl
    S = spd("g18_full")
    rng = np.random.default_rng(17)
    B = S.s[:, None] * rng.standard_normal((S.n, max(NRHS)))
    B[:, 0] = S.rhs
    p = S.perm
    Bp = B[p]
    X = sl.cho_solve((S.Ld, True), Bp)
    X += sl.cho_solve((S.Ld, True), Bp - S.PAP @ X)
    Xref = np.empty_like(X)
    Xref[p] = X
    return S, B, Xref


def _block(B, ld):
    return Guarded(B.shape[0], B.shape[1], ld, values=B)


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
def test_block_solve_chunk_edges_padding_and_in_place(f32, block_ref):
    import cholesky_amd as ca
    S, Ball, Xref = block_ref
    n, ld = S.n, S.n + 3
    dev = ca.Device(S.plan, 0)
    a = _factor(dev, f32)
    u = U32 if f32 else U64
    for k in NRHS:
        B = _block(Ball[:, :k], ld)
        X = Guarded(n, k, ld)
        snap = B.snapshot()
        dev.solve_nrhs(a.t, B.t, X.t)
        dev.sync()
        B.assert_unchanged(snap, f"B, nrhs {k}")
        X.assert_guards(f"X, nrhs {k}")           # guards and padding rows: the pattern; B's NaN padding did not reach X
        x = X.numpy()
        for j in range(k):
            assert S.forward_error(x[:, j], Xref[:, j]) <= S.tol_forward(u), (k, j)
        dev.solve_nrhs(a.t, B.t, B.t)             # in place
        dev.sync()
        B.assert_guards(f"B in place, nrhs {k}")
        x = B.numpy()
        for j in range(k):
            assert S.forward_error(x[:, j], Xref[:, j]) <= S.tol_forward(u), ("in place", k, j)
        if f32:
            B = _block(Ball[:, :k], ld)
            X = Guarded(n, k, ld)
            snap = B.snapshot()
            tol = 1e-12
            it, rel = dev.solve_refine_nrhs(a.t, B.t, X.t, max_iter=MAX_ITER, tol=tol)
            B.assert_unchanged(snap, f"B refine, nrhs {k}")
            X.assert_guards(f"X refine, nrhs {k}")
            assert (rel <= tol).all() and it <= S.refine_iterations(tol), (k, it, rel.max())
            x = X.numpy()
            for j in range(k):
                assert S.forward_error(x[:, j], Xref[:, j]) <= S.tol_forward(), ("refine", k, j)


# ------------------------------------------------------------------------------------------------
# f. sharded: rank arenas (owned ranges and the aliased scratch chunk poisoned), distributed solve and refinement
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sharded_ref(tmp_path_factory):
    import cholesky_amd as ca
    orc.use_own_kernels()
    prob = ca.Problem(20, 20, 20, 4, 32)
    m, o, c, _ = prob.write(os.path.join(tmp_path_factory.mktemp("sharded"), "gen"))
    O = orc.Oracle(m, o, c)
    O.factor()
    b = prob.rhs()
    return prob.plan(), b, O.solve(b)


@pytest.mark.parametrize("dist_top", [0, 1])
@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("world", [2, 4])
def test_sharded_rank_arenas_solve(world, f32, dist_top, sharded_ref):
    import cholesky_amd as ca
    from cholesky_amd.device import factor_multi, solve_multi, solve_refine_multi
    plan, bvec, xo = sharded_ref
    devs, arenas = [], []
    for r in range(world):
        dev = ca.Device(plan, 0)
        dev.set_option("dist_top", dist_top)
        dev.set_partition(r, world)
        a = dev.alloc_arena(4 if f32 else 8)
        (dev.fill_f32 if f32 else dev.fill)(a)
        devs.append(dev)
        arenas.append(a)
    factor_multi(devs, arenas, local=True)
    for dev in devs:
        assert dev.info() == (0, 0)
    b = Guarded(plan.n, values=bvec)
    snap = b.snapshot()
    xs = [Guarded(plan.n) for _ in range(world)]
    if f32:
        iters, rel = solve_refine_multi(devs, arenas, [b.t] * world, [x.t for x in xs], max_iter=20, tol=1e-13, local=True)
        assert rel <= 1e-12 and iters <= 8, (iters, rel)
    else:
        solve_multi(devs, arenas, [b.t] * world, [x.t for x in xs], local=True)
    b.assert_unchanged(snap, "b")
    scale = max(1.0, np.abs(xo).max())
    for r, x in enumerate(xs):
        x.assert_guards(f"x of rank {r}")
        assert np.abs(x.numpy() - xo).max() <= (1e-10 if f32 else 1e-9) * scale, r
    for a in arenas:
        a.free()
