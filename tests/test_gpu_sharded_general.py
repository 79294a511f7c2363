"""The multi-rank factor and solves on general SPD inputs (tests/spd_inputs.py, tests/tree_inputs.py), replicated and distributed top, fp64 and fp32.

Every other multi-rank GPU test factors a constant-coefficient grid Laplacian -- sibling subtrees are mirror images, every update product has one
sign, the top separators are planes of a few fixed block counts -- and compares with the library's own single-GPU result.  Here the inputs have
log-uniform mixed-sign values on unbalanced trees, so an ownership or ordering error between sibling subtrees cannot cancel, and the references are
independent: the dense LAPACK factor, the CPU oracle and the long-double-refined dense solution, at spd_inputs' derived bounds (tol_* of k, u, kappa).

  tree_over    two column blocks for four ranks: ranks without a pivot column at a top level (193 = 112 + 81, 145 = 80 + 65)
  tree_skew    top separators of one column; at world 8 every rank owns one leaf (1 .. 289 columns) and one rank owns no piece of the exchange
  tree_top     top separators of four and three column blocks (433 = 3 x 112 + 97, 289 = 2 x 112 + 65) next to one of a single column: the cyclic
               owner rule wraps, a super-block of three column blocks ends inside the root, at world 2 a rank owns blocks 0 and 2 or 1 and 3
  g16_subset   a grid's balanced subtrees with a random-subset stencil (n = 2048)

All of them have "tiles" (row-compacted, disjoint between siblings) or missing couplings into the top, over which the path-aware contributor mask of
the exchange and the nb x ld broadcast pieces have to be right.

Everything runs in one process over the local communicator (at most 8 rank objects and one single-GPU object on the one GPU), under CHOLAMD_POISON=1,
on rank arenas of cholamd_device_alloc_arena: the ranges of the other ranks' panels alias the poisoned scratch chunk, so a read of a panel the rank
does not own shows as NaN.  Vectors are `guarded.Guarded` buffers.  Each test prints its errors as fractions of their bounds ("margin" lines)."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tree_inputs as ti  # noqa: E402
from guarded import Guarded  # noqa: E402
from sharded import assemble, gather_factor, panel_owners, panel_ranges  # noqa: E402
from spd_inputs import U32, U64  # noqa: E402
from test_gpu_factor_query import logdet_tol  # noqa: E402
from test_gpu_general_spd import _diag_index, _ids  # noqa: E402
from test_gpu_trees import MAX_ITER, _block_refs  # noqa: E402

CASES = [("tree_over", 2), ("tree_over", 4), ("tree_skew", 2), ("tree_skew", 4), ("tree_skew", 8), ("tree_top", 2), ("tree_top", 4), ("g16_subset", 4)]
CASE_IDS = [f"{nm}-w{w}" for nm, w in CASES]
PRECISIONS, PIDS = [False, True], ["fp64", "fp32"]
TOL_REFINE = 1e-12
_REFS = {}


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("CHOLAMD_POISON", "1")
    for v in ("CHOLAMD_SOLVE_NO_BAND", "CHOLAMD_SOLVE_NO_INV256", "CHOLAMD_SOLVE_REFERENCE_SHAPE"):
        monkeypatch.delenv(v, raising=False)


@pytest.fixture(scope="module")
def spd(tmp_path_factory):
    return lambda name: ti.cached(tmp_path_factory, name)


def _second_rhs(S, name):
    """A second right-hand side and its reference solution (a column of test_gpu_trees' block references), once per input."""
    if name not in _REFS:
        B, Xref = _block_refs(S, 2)
        _REFS[name] = (B[:, 1].copy(), Xref[:, 1].copy())
    return _REFS[name]


def _margin(what, measure, err, tol):
    print(f"margin {what} {measure}: {err:.3e} / {tol:.3e} = {err / tol:.3e}")
    return err


@contextlib.contextmanager
def _ranks(S, world, dist_top, f32, opts=None):
    """The `world` rank objects of S's plan (options set before the partition) and their rank arenas, freed on the way out."""
    import cholesky_amd as ca
    devs, arenas = [], []
    try:
        for r in range(world):
            dev = ca.Device(S.plan, 0)
            dev.set_option("dist_top", dist_top)
            for k, v in (opts or {}).items():
                dev.set_option(k, v)
            dev.set_partition(r, world)
            devs.append(dev)
            arenas.append(dev.alloc_arena(4 if f32 else 8))
        yield devs, arenas
    finally:
        for a in arenas:
            a.free()


def _fill(devs, arenas, f32):
    for dev, a in zip(devs, arenas):
        (dev.fill_f32 if f32 else dev.fill)(a)
    for dev in devs:
        dev.sync()


def _parts(S, arenas):
    """The ranks' arenas as host arrays in their own element type (the ranges a rank does not own: whatever the scratch chunk holds)."""
    assert S.plan.arena_doubles % 2 == 0     # RankArena.numpy copies whole doubles
    return [a.numpy() for a in arenas]


def _check_factor(S, devs, arenas, f32, what):
    """3b: info, identical tails, and the factor assembled from the owners against the dense factor, the oracle and A."""
    from cholesky_amd import parallel
    plan, world = S.plan, len(devs)
    for r, dev in enumerate(devs):
        assert dev.info() == (0, 0), (what, r, dev.info())
    tail = parallel.tail_offset(plan, world)
    parts = _parts(S, arenas)
    for r in range(1, world):
        assert np.array_equal(parts[r][tail:], parts[0][tail:]), (what, r)           # every rank ends with the same complete top, bit for bit
    L = np.tril(plan.arena_to_dense(assemble(plan, parts, world).astype(np.float64)))
    u = U32 if f32 else U64
    row_d = _margin(what, "row_error vs dense", S.row_error(L), S.tol_factor(u))
    row_o = _margin(what, "row_error vs oracle", S.row_error(L, S.Lo), S.tol_factor(u))
    rec = _margin(what, "reconstruction", S.reconstruction(L), S.tol_reconstruction(u))
    assert row_d <= S.tol_factor(u), what
    assert row_o <= S.tol_factor(u), what
    assert rec <= S.tol_reconstruction(u), what
    if not f32:
        assert np.array_equal(L != 0, S.Lo != 0), what                                # the oracle's zero pattern, entry for entry


def _factor(devs, arenas, f32):
    from cholesky_amd.device import factor_multi
    _fill(devs, arenas, f32)
    factor_multi(devs, arenas, local=True)


def _check_x(S, x, bvec, xref, what, backward=True):
    if backward:
        be = _margin(what, "backward_error", S.backward_error(x, bvec), S.tol_backward())
        assert be <= S.tol_backward(), what
    fe = _margin(what, "forward_error", S.forward_error(x, xref), S.tol_forward())
    assert fe <= S.tol_forward(), what


def _check_refined(S, x, it, rel, what):
    limit = S.refine_iterations(TOL_REFINE)
    print(f"margin {what} refinement: {it} of {limit} iterations, relres {rel:.3e}")
    assert rel <= TOL_REFINE and it <= limit, (what, it, rel, limit)
    true = S.true_relres(x, S.rhs)
    assert abs(rel - true) <= 1e-13 + 0.5 * true, (what, rel, true)                   # the residual it reports is the true one
    fe = _margin(what, "forward_error", S.forward_error(x), S.tol_forward())
    assert fe <= S.tol_forward(), what


# ------------------------------------------------------------------------------------------------
# a. rank-aware fill
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("dist_top", [0, 1])
@pytest.mark.parametrize("name,world", CASES, ids=CASE_IDS)
def test_rank_aware_fill(name, world, dist_top, f32, spd):
    """The ranks' fills tile the single-GPU fill: the tails add up to its tail bit for bit, an element of the tail starts from A on one rank at
    most (rank 0 with the top replicated, the column block's owner with it distributed), and under the cut a rank's own panels are the single
    fill's."""
    import torch
    import cholesky_amd as ca
    from cholesky_amd import parallel
    S = spd(name)
    plan = S.plan
    one = ca.Device(plan, 0)
    ref = Guarded(plan.arena_doubles, dtype=torch.float32 if f32 else torch.float64)
    (one.fill_f32 if f32 else one.fill)(ref.t)
    one.sync()
    ref.assert_guards("single-GPU arena")
    full = ref.t.cpu().numpy()
    tail = parallel.tail_offset(plan, world)
    with _ranks(S, world, dist_top, f32) as (devs, arenas):
        assert all(dev.tail_offset() == tail for dev in devs) and 0 < tail < plan.arena_doubles
        assert all(dev.dist_top_active() == bool(dist_top) for dev in devs)
        _fill(devs, arenas, f32)
        parts = _parts(S, arenas)
    assert all(p.dtype == full.dtype for p in parts) and full[tail:].any()
    total = parts[0][tail:].copy()
    for p in parts[1:]:
        total += p[tail:]                                  # exact: at most one term is not zero
    assert np.array_equal(total, full[tail:])
    nonzero = sum((p[tail:] != 0).astype(np.int64) for p in parts)
    assert (nonzero <= 1).all()
    if not dist_top:
        assert not any(p[tail:].any() for p in parts[1:])  # replicated top: A's entries of the top start on rank 0
    elif not f32:                                          # the fp64 schedule's pieces are the plan's: a piece starts from A on its owner only
        for off, count, owner, _ in plan.exchange_pieces(world, 1).tolist():
            for r in range(world):
                if r != owner:
                    assert not parts[r][off:off + count].any(), (off, owner, r)
    owner, ranges = panel_owners(plan, world), panel_ranges(plan)
    for s, (lo, hi) in ranges.items():
        if hi <= tail:
            assert np.array_equal(parts[owner[s]][lo:hi], full[lo:hi]), s


# ------------------------------------------------------------------------------------------------
# b. factor
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("dist_top", [0, 1])
@pytest.mark.parametrize("name,world", CASES, ids=CASE_IDS)
def test_factor_multi_on_general_inputs(name, world, dist_top, f32, spd):
    S = spd(name)
    what = f"{name} w{world} dist_top={dist_top} {PIDS[f32]}"
    with _ranks(S, world, dist_top, f32) as (devs, arenas):
        _factor(devs, arenas, f32)
        _check_factor(S, devs, arenas, f32, what)


# ------------------------------------------------------------------------------------------------
# c. solves with the factor left on the ranks
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("dist_top", [0, 1])
@pytest.mark.parametrize("name,world", CASES, ids=CASE_IDS)
def test_solves_with_the_factor_on_the_ranks(name, world, dist_top, f32, spd):
    """fp64: cholamd_solve_multi, twice through the same lists; fp32: cholamd_solve_refine_multi.  Every rank's x against the long-double-refined
    dense solution, not against the single-GPU solve."""
    from cholesky_amd.device import solve_multi, solve_refine_multi
    S = spd(name)
    n = S.n
    what = f"{name} w{world} dist_top={dist_top} {PIDS[f32]}"
    with _ranks(S, world, dist_top, f32) as (devs, arenas):
        _factor(devs, arenas, f32)
        for r, dev in enumerate(devs):
            assert dev.info() == (0, 0), (what, r)
        b = Guarded(n, values=S.rhs)
        snap = b.snapshot()
        xs = [Guarded(n) for _ in range(world)]              # x starts as the NaN pattern
        if f32:
            it, rel = solve_refine_multi(devs, arenas, [b.t] * world, [x.t for x in xs], max_iter=MAX_ITER, tol=TOL_REFINE, local=True)
        else:
            solve_multi(devs, arenas, [b.t] * world, [x.t for x in xs], local=True)
        b.assert_unchanged(snap, "b")
        for r, x in enumerate(xs):
            x.assert_guards(f"x of rank {r}")
            if f32:
                _check_refined(S, x.numpy(), it, rel, f"{what} rank {r}")
            else:
                _check_x(S, x.numpy(), S.rhs, S.x_ref, f"{what} rank {r}")
        if f32:
            return
        b2v, x2ref = _second_rhs(S, name)
        b2 = Guarded(n, values=b2v)
        snap = b2.snapshot()
        xs = [Guarded(n) for _ in range(world)]
        solve_multi(devs, arenas, [b2.t] * world, [x.t for x in xs], local=True)
        b2.assert_unchanged(snap, "second b")
        for r, x in enumerate(xs):
            x.assert_guards(f"second x of rank {r}")
            _check_x(S, x.numpy(), b2v, x2ref, f"{what} second rhs rank {r}")


# ------------------------------------------------------------------------------------------------
# d. gather, then the full-tree entry points on rank 0
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("name,world", CASES, ids=CASE_IDS)
def test_gathered_factor_serves_rank_zero(name, world, f32, spd):
    """cholamd_gather_factor / _f32, then solve, logdet (fp64) or solve_refine (fp32) of rank 0's partitioned object on its now complete arena.
    One dist_top value per case: distributed at world 4, replicated at world 2 and 8."""
    S = spd(name)
    n = S.n
    dist_top = 1 if world == 4 else 0
    what = f"{name} w{world} dist_top={dist_top} {PIDS[f32]} gathered"
    with _ranks(S, world, dist_top, f32) as (devs, arenas):
        _factor(devs, arenas, f32)
        for r, dev in enumerate(devs):
            assert dev.info() == (0, 0), (what, r)
        gather_factor(devs, arenas, f32)
        b, x = Guarded(n, values=S.rhs), Guarded(n)
        snap = b.snapshot()
        if f32:
            it, rel = devs[0].solve_refine(arenas[0], b.t, x.t, max_iter=MAX_ITER, tol=TOL_REFINE)
        else:
            devs[0].solve(arenas[0], b.t, x.t)
        devs[0].sync()
        b.assert_unchanged(snap, "b")
        x.assert_guards("x")
        if f32:
            _check_refined(S, x.numpy(), it, rel, what)
        else:
            _check_x(S, x.numpy(), S.rhs, S.x_ref, what)
            ld = devs[0].logdet(arenas[0])
            ref = 2.0 * float(np.sum(np.log(np.diag(S.Ld))))
            tol = logdet_tol(S.k, S.kappa, n, U64)
            _margin(what, "logdet", abs(ld - ref), tol)
            assert abs(ld - ref) <= tol, (what, ld, ref)


# ------------------------------------------------------------------------------------------------
# e. kernel-path switches under the distributed top
# ------------------------------------------------------------------------------------------------
def _assert_macro_tiles(S, world, f32):
    """Every rank's lists hold macro-tile tasks under mt_min_tiles = 1 (Plan.level_mt_classes, summed over the levels)."""
    for r in range(world):
        n = sum(S.plan.level_mt_classes(lvl, 1, 1, f32, r, world, 1)["tasks"] for lvl in range(S.plan.levels))
        assert n > 0, (world, r, f32)


@pytest.mark.parametrize("opts", [{"trsm_wt_min": 1}, {"fuse": 0}, {"super_blocks": 1}, {"mt_min_tiles": 1}], ids=_ids)
def test_kernel_path_switches_under_the_distributed_top(opts, spd):
    """tree_top at world 4, fp64: the owners' strips through the throughput TRSM, POTRF and TRSM as launches of their own, rank-nb trailing
    updates instead of super-blocks, and the updates on 64 x 64 macro tiles -- each with the column blocks of the top spread over the ranks."""
    S = spd("tree_top")
    if "mt_min_tiles" in opts:
        _assert_macro_tiles(S, 4, False)
    with _ranks(S, 4, 1, False, opts) as (devs, arenas):
        _factor(devs, arenas, False)
        _check_factor(S, devs, arenas, False, f"tree_top w4 dist_top=1 fp64 {_ids(opts)}")


@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("world", [2, 4])
def test_macro_tiles_under_the_distributed_top(world, f32, spd):
    """tree_top with mt_min_tiles = 1 at worlds 2 and 4, fp64 and fp32: SYRK targets cut at the top separators' column blocks reach the macro-tile
    kernels with an origin of their own (ar, br no multiples of 64; tests/test_update_mt_host.py counts them)."""
    S = spd("tree_top")
    _assert_macro_tiles(S, world, f32)
    with _ranks(S, world, 1, f32, {"mt_min_tiles": 1}) as (devs, arenas):
        _factor(devs, arenas, f32)
        _check_factor(S, devs, arenas, f32, f"tree_top w{world} dist_top=1 {'fp32' if f32 else 'fp64'} mt_min_tiles=1")


# ------------------------------------------------------------------------------------------------
# f. pivot failure on a partitioned object
# ------------------------------------------------------------------------------------------------
PIVOTS = {"leaf_last": (7, 129, 128), "root_block2": (1, 433, 112), "one_column": (3, 1, 0)}     # (heap index, columns, failing column) in tree_top


@pytest.mark.parametrize("dist_top", [0, 1])
@pytest.mark.parametrize("where,f32", [("leaf_last", False), ("root_block2", False), ("root_block2", True), ("one_column", False)],
                         ids=["leaf_last-fp64", "root_block2-fp64", "root_block2-fp32", "one_column-fp64"])
def test_pivot_failure_on_a_partitioned_object(where, f32, dist_top, spd):
    """A'_kk = A_kk - 1.5 L_kk^2 (test_pivot_failure_at_the_thresholds' construction) on tree_top at world 4: the last column of a leaf, the first
    column of the root's second column block, the one-column separator.  The value reaches every rank object through set_values (the same value
    array) and fill.  info belongs to the device object: every rank that factors column k reports exactly (k - offset + 1, separator); a rank
    that does not reports (0, 0) or -- NaN reached it through the exchange or a broadcast -- a later pivot; so the smallest position over the
    ranks is the first failing pivot, LAPACK's.  Who factors k comes from the library's lists: the subtree's owner under the cut; in the top
    every rank (replicated) or the owner of the exchange piece that holds the diagonal element (distributed; the fp32 schedule cuts 433 columns
    into the same four blocks of 112, 112, 112 and 97 as the fp64 one: blocks of at most 128 against 144).  Afterwards the original values give
    (0, 0) on every rank and a factor within the bounds."""
    from scipy.linalg import lapack
    S = spd("tree_top")
    P, world = S.plan, 4
    heap, size, col = PIVOTS[where]
    lbl = int(P.tree[heap - 1])
    off = int(P.sep_offsets[lbl - 1])
    assert P.sep_sizes[lbl - 1] == size and 0 <= col < size
    k = off + col
    newv = S.PAP[k, k] - 1.5 * S.Ld[k, k] ** 2
    Ap = S.PAP.copy()
    Ap[k, k] = newv
    assert lapack.dpotrf(Ap, lower=1)[1] == k + 1
    # the value arrays, in the order of the matrix file (plan.entries())
    o = np.lexsort((S.row, S.col))
    row, cl = P.entries()
    assert np.array_equal(row, S.row[o]) and np.array_equal(cl, S.col[o])
    good = np.ascontiguousarray(S.val[o])
    dof = int(P.perm[k])
    e = np.nonzero((row == dof) & (cl == dof))[0]
    assert len(e) == 1 and good[e[0]] == S.PAP[k, k]
    bad = good.copy()
    bad[e[0]] = newv
    # who factors column k
    d = world.bit_length() - 1
    if heap.bit_length() - 1 >= d:
        factoring = {panel_owners(P, world)[lbl]}
    elif dist_top == 0:
        factoring = set(range(world))
    else:
        idx = _diag_index(P, P.fill_host(), k)
        rows = [p for p in P.exchange_pieces(world, 1).tolist() if p[0] <= idx < p[0] + p[1]]
        assert len(rows) == 1 and rows[0][3] == heap
        factoring = {rows[0][2]}
    expect = (col + 1, lbl)
    what = f"tree_top w4 dist_top={dist_top} {PIDS[f32]} pivot {where}"
    with _ranks(S, world, dist_top, f32) as (devs, arenas):
        for dev in devs:
            dev.set_values(bad)
        _factor(devs, arenas, f32)                         # factor_multi returns and every rank's sync completes
        infos = [dev.info() for dev in devs]
        print(f"{what}: column {k}, factored by {sorted(factoring)}, info {infos}")
        positions = []
        for r, (c, s) in enumerate(infos):
            if r in factoring:
                assert (c, s) == expect, (what, r, infos, expect)
            else:
                assert (c, s) == (0, 0) or (c > 0 and int(P.sep_offsets[s - 1]) + c - 1 > k), (what, r, infos, expect)
            if c > 0:
                positions.append(int(P.sep_offsets[s - 1]) + c - 1)
        assert min(positions) == k
        for dev in devs:
            dev.set_values(good)
        _factor(devs, arenas, f32)
        _check_factor(S, devs, arenas, f32, what + ", good values again")
