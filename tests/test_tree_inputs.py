"""CPU tests of the synthetic-tree inputs (tests/tree_inputs.py), mirroring test_spd_inputs.py: the files and the arrays give the same plan, the
host fill, the CPU oracle, the solve's skipped entries, the program launch's self-check and the factor's diagonal list on trees whose separator
sizes sit on the kernels' size thresholds -- and a sensitivity test: one dropped 16 x 16 contribution fails the measures the GPU tests apply."""
import numpy as np
import pytest

import spd_inputs as si
import tree_inputs as ti

ALL = ti.NAMED + ti.SINGLE + ti.TOP + ti.DEEP


@pytest.fixture(scope="module")
def spd(tmp_path_factory):
    return lambda name: ti.cached(tmp_path_factory, name)


def test_named_trees_are_the_suites_inputs():
    assert si.NAMES[-len(ti.NAMED):] == ti.NAMED and not set(ti.SINGLE + ti.TOP + ti.DEEP) & set(si.NAMES)
    assert si.NAMES.index("g7_ragged") == 9             # the inputs before the trees keep their places, and so their seeds


@pytest.mark.parametrize("name", ALL)
def test_files_and_arrays_give_the_same_plan(name, spd):
    S = spd(name)
    T, P = S.tree, S.plan
    ti.assert_same_plan(P, S.plan_arrays)
    assert np.array_equal(P.perm, T.perm) and np.array_equal(P.sep_sizes, T.sep_sizes)
    assert P.levels == T.levels and [int(P.sep_sizes[P.tree[h] - 1]) for h in range(P.nsep)] == ti.TREES[name]["sizes"]
    assert not np.array_equal(P.perm, np.arange(P.n))   # original order is not permuted order
    if ti.TREES[name]["tile"] == "random":
        b0 = np.concatenate([b[0] for b in T.boundaries.values()])
        assert (b0 % 16 != 0).any() and any((np.diff(b[0]) == 1).any() for b in T.boundaries.values() if b[0][-1] >= 3)


@pytest.mark.parametrize("name", ALL)
def test_builder_gives_spd_matrices_the_host_fill_reproduces(name, spd):
    S = spd(name)
    assert S.plan.dropped == 0 and S.plan_arrays.dropped == 0
    assert np.all(np.isfinite(S.Ld)) and np.all(np.diag(S.Ld) > 0)
    assert np.array_equal(S.A, S.A.T)
    off = S.A[~np.eye(S.n, dtype=bool)]
    assert (off > 0).any() and (off < 0).any()
    H = S.plan.arena_to_dense(S.plan.fill_host())
    assert np.array_equal(np.tril(H), np.tril(S.PAP))
    # the guard rails of the generator: the tolerances say something, and refine_iterations is defined
    assert S.kappa < 1e3
    assert S.tol_forward(si.U32) < 0.5


@pytest.mark.parametrize("position,leaf", [("leaf", "dense"), ("leaf", ("band", 17)), ("middle", "dense"), ("root", "dense")],
                         ids=["leaf_dense", "leaf_band17", "middle", "root"])
def test_sweep_inputs_hold_the_guard_rails(position, leaf, tmp_path):
    """Every input of test_gpu_trees' sweep (the same generator, other sizes and seeds), without the oracle: the size sits where it should, nothing
    is dropped, files and arrays agree (SPD asserts it), the guard rails hold and the program launch's self-check is live."""
    heap = {"leaf": 4, "middle": 2, "root": 1}[position]
    for s in ti.SWEEP_SIZES:
        S = ti.sweep(tmp_path, position, s, leaf, oracle=False)
        P = S.plan
        assert S.n == s + 142 and P.dropped == 0 and P.sep_sizes[P.tree[heap - 1] - 1] == s
        assert S.kappa < 1e3 and S.tol_forward(si.U32) < 0.5, (position, s, S.kappa)
        off = S.A[~np.eye(S.n, dtype=bool)]
        assert (off > 0).any() and (off < 0).any()
        for follow in (1, 0):
            P.program_check(follow, 64)


@pytest.mark.parametrize("name", ALL)
def test_oracle_factor_matches_dense_cholesky(name, spd):
    S = spd(name)
    assert S.row_error(S.Lo) <= S.tol_factor()
    assert S.reconstruction(S.Lo) <= S.tol_reconstruction()
    assert not S.Lo[S.Ld == 0].any()


@pytest.mark.parametrize("name", ALL)
def test_program_launch_check_on_trees(name, spd):
    P = spd(name).plan
    for follow in (1, 0):
        for workers in (256, 32, 4):
            P.program_check(follow, workers)
    for split in (64, 96, 192):
        P.program_check_opts(split_min=split, split_nb=split)


@pytest.mark.parametrize("name", ALL)
def test_what_the_solve_skips_is_zero_in_the_factor_of_trees(name, spd):
    S = spd(name)
    P = S.plan
    for level in range(P.levels):
        seps, runs = P.solve_skips(level)
        if level < P.levels - 1:
            assert not seps[:, 2].any() and not runs[:, 4].any()
            continue
        for Lf in (S.Lo, S.Ld):
            for off, n, band in seps:
                if band > 0:
                    D = Lf[off:off + n, off:off + n]
                    i, j = np.indices(D.shape)
                    assert not D[i - j > band].any()
            for x_off, m, y_off, n, c_lo in runs:
                assert 0 <= c_lo <= n and c_lo % 16 == 0
                assert not Lf[x_off:x_off + m, y_off:y_off + c_lo].any()


@pytest.mark.parametrize("name", ALL)
def test_diag_list_covers_every_position_once(name, spd):
    S = spd(name)
    P = S.plan
    a_off, cols, lda, x_off, sep, prefix = P.diag_list()
    host = P.fill_host()
    seen = np.zeros(P.n, dtype=np.int64)
    got = np.full(P.n, np.nan)
    for i in range(len(a_off)):
        j = np.arange(cols[i], dtype=np.int64)
        seen[x_off[i] + j] += 1
        got[x_off[i] + j] = host[a_off[i] + j * (int(lda[i]) + 1)]
    assert (seen == 1).all()
    assert np.array_equal(got, np.diag(S.PAP))            # x_off counts permuted positions


@pytest.mark.parametrize("name", ALL)
def test_sparse_arena_reader_equals_the_dense_one(name, spd):
    S = spd(name)
    host = S.plan.fill_host()
    Ls = si.arena_to_sparse(S.plan, host)
    assert np.array_equal(Ls.toarray(), np.tril(S.plan.arena_to_dense(host)))
    assert np.array_equal(Ls.toarray(), np.tril(S.PAP))


@pytest.mark.parametrize("name", ti.WITH_TILES + ti.TOP)
def test_tiles_couplings_are_row_compacted(name, spd):
    S = spd(name)
    assert S.tree.untouched_tiles > 0 and "tiles" in S.tree.kinds.values()
    assert S.plan.arena_doubles < S.plan.arena_dense_doubles
    gone = 0
    for b in S.plan.blocks:
        r, c = int(b[0]), int(b[1])
        if r != c:
            gone += int((S.plan.block_tile_map(r, c) < 0).sum())
    assert gone > 0


def test_tree_top_has_top_separators_of_three_and_four_column_blocks(spd):
    """What tree_top is for, read from the library's own piece list of the distributed top: the root is cut in 112 + 112 + 112 + 97 columns and
    heap index 2 in 112 + 112 + 65; at world 4 the cyclic owner rule wraps (ranks 1, 2, 3, 0 and 2, 3, 0) and the one-column separator is rank
    3's; at world 2 each rank owns two blocks of the root that are not neighbours."""
    S = spd("tree_top")
    P = S.plan
    assert S.n == 967 and S.tree.untouched_tiles > 0
    ld = {int(b[1]): int(b[6]) for b in P.blocks if b[0] == b[1]}

    def cut(world, heap):
        rows = P.exchange_pieces(world, 1)
        rows = rows[rows[:, 3] == heap]
        rows = rows[np.argsort(rows[:, 0])]
        assert (rows[:, 1] % ld[int(P.tree[heap - 1])] == 0).all()
        return (rows[:, 1] // ld[int(P.tree[heap - 1])]).tolist(), rows[:, 2].tolist()

    assert cut(4, 1) == ([112, 112, 112, 97], [1, 2, 3, 0])
    assert cut(4, 2) == ([112, 112, 65], [2, 3, 0])
    assert cut(4, 3) == ([1], [3])
    assert cut(2, 1) == ([112, 112, 112, 97], [1, 0, 1, 0])


def test_a_dropped_tile_contribution_fails_the_measures(spd):
    """Dense numpy's factor of tree_over with one separator's pivot recomputed from a Schur complement that lacks one 16 x 16 product
    L(I, K) L(I, K)^T of a descendant's panel (16 rows I of the separator, 16 columns K of the descendant, structurally non-zero): row_error and
    reconstruction then exceed their fp64 tolerances by orders of magnitude (4.2e-4 against 1.6e-12, 6.5e-5 against 1.5e-11), so an fp64 kernel
    that dropped a tile could not pass.  (The fp32 bound on the factor, 8.6e-4 here, is wider than this one tile's 4.2e-4: for the fp32 factor
    it is the fp64 paths' shared lists and the zero pattern that stand guard, not the bound.)"""
    S = spd("tree_over")
    P = S.plan
    mid = int(P.tree[1])                                   # heap index 2: the separator of 177 columns
    off, m = int(P.sep_offsets[mid - 1]), int(P.sep_sizes[mid - 1])
    assert m == 177
    leaf = int(P.tree[4])                                  # heap index 5, a child: 273 columns
    lo, w = int(P.sep_offsets[leaf - 1]), int(P.sep_sizes[leaf - 1])
    panel = S.Ld[off:off + m, lo:lo + w]
    I = next(t for t in range(m // 16) if panel[16 * t:16 * t + 16, w - 16:].all())
    X = panel[16 * I:16 * I + 16, w - 16:]
    assert np.count_nonzero(X) == 256
    D = S.Ld[off:off + m, off:off + m]
    C = D @ D.T                                            # the separator's block after every update
    C[16 * I:16 * I + 16, 16 * I:16 * I + 16] += X @ X.T   # ... with one update left out
    L = S.Ld.copy()
    L[off:off + m, off:off + m] = np.linalg.cholesky(C)
    assert S.row_error(S.Ld) == 0.0
    row, rec = S.row_error(L), S.reconstruction(L)
    print(f"dropped tile: row_error = {row:.3g} (tol {S.tol_factor():.3g}), reconstruction = {rec:.3g} (tol {S.tol_reconstruction():.3g})")
    assert row > 1e3 * S.tol_factor() and rec > 1e3 * S.tol_reconstruction()


def test_tree_deep_is_seven_levels_of_dense_couplings(spd):
    """What tree_deep is for: 127 separators on seven levels (the separator file's level field is still one digit), every one coupled to every
    ancestor, three in four leaves to all 80 rows of the root and every fourth to its first 48 only -- so the root's tile pairs collect 64 and 48
    sources from the leaf level (tests/test_update_mt_host.py counts the lists)."""
    S = spd("tree_deep")
    T, P = S.tree, S.plan
    assert (P.levels, P.nsep, S.n) == (7, 127, 1634) and T.heap_sizes[:3] == [80, 40, 33]
    assert open(S.ord).readline().split() == ["7", "127"]
    assert all(T.kinds[c >> j, c] != "none" for c in range(2, 128) for j in range(1, c.bit_length()))
    rows = [T.kinds[1, c] for c in range(64, 128)]
    assert rows.count(("rows", 48)) == 16 and rows.count(("random", 0.5)) == 48
    root = P.sep_offsets[P.tree[0] - 1]
    for c in (64, 67):
        lo, w = int(P.sep_offsets[P.tree[c - 1] - 1]), T.heap_sizes[c - 1]
        panel = S.PAP[root:root + 80, lo:lo + w]
        assert panel[:48].any() and panel[48:].any() == (c % 4 != 3)


def test_a_dropped_tile_contribution_into_the_root_of_tree_deep_fails_the_measures(spd):
    """The argument of test_a_dropped_tile_contribution_fails_the_measures for tree_deep's root, which collects a contribution from each of its 126
    descendants: the root's pivot recomputed from a Schur complement that lacks ONE 16 x 16 product of ONE leaf's panel (the last 16 columns of
    heap index 64, 16 rows of the root) exceeds the fp64 tolerances on row error and reconstruction by more than 1e3 -- a macro-tile kernel that
    lost one source at the restart between two descriptor batches could not pass."""
    S = spd("tree_deep")
    P = S.plan
    root = int(P.tree[0])
    off, m = int(P.sep_offsets[root - 1]), int(P.sep_sizes[root - 1])
    leaf = int(P.tree[63])
    lo, w = int(P.sep_offsets[leaf - 1]), int(P.sep_sizes[leaf - 1])
    assert m == 80 and 16 <= w <= 21
    panel = S.Ld[off:off + m, lo:lo + w]
    I = next(t for t in range(m // 16) if panel[16 * t:16 * t + 16, w - 16:].all())
    X = panel[16 * I:16 * I + 16, w - 16:]
    D = S.Ld[off:off + m, off:off + m]
    C = D @ D.T
    C[16 * I:16 * I + 16, 16 * I:16 * I + 16] += X @ X.T
    L = S.Ld.copy()
    L[off:off + m, off:off + m] = np.linalg.cholesky(C)
    row, rec = S.row_error(L), S.reconstruction(L)
    print(f"dropped tile, tree_deep: row_error = {row:.3g} (tol {S.tol_factor():.3g}), reconstruction = {rec:.3g} (tol {S.tol_reconstruction():.3g}); "
          f"fp32 tol {S.tol_factor(si.U32):.3g}")
    assert row > 1e3 * S.tol_factor() and rec > 1e3 * S.tol_reconstruction()
