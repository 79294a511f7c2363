"""Host side of the Schur complement on the top of the tree (cholamd_plan_schur_*): the kept set against the plan's own tree, the records of the gather
against the block table and the tile maps, the CPU gather against the dense image of the arena, the argument errors -- no device needed.

Nothing is eliminated here: the arena is the plain host fill, so S = A_TT and every comparison is exact."""
import numpy as np
import pytest

from conftest import CASES, case_paths

GENERATED = {"gen_20x20": (20, 20, 1, 4, 16), "gen_12x12x12": (12, 12, 12, 4, 16)}
NAMES = list(CASES) + list(GENERATED)


@pytest.fixture(scope="module")
def ca():
    import cholesky_amd
    return cholesky_amd


@pytest.fixture(scope="module")
def plans(ca):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = ca.Plan(*case_paths(name)[:3]) if name in CASES else ca.Problem(*GENERATED[name][:3], levels=GENERATED[name][3], tile=GENERATED[name][4]).plan()
        return cache[name]
    return get


def ks(plan):
    return range(1, min(3, plan.levels - 1) + 1)


def kept_labels(plan, k):
    return [int(s) for s in plan.tree[: (1 << k) - 1]]


@pytest.mark.parametrize("name", NAMES)
def test_size_and_dofs_follow_the_tree(plans, name):
    plan = plans(name)
    sizes, offs, perm, n = plan.sep_sizes, plan.sep_offsets, plan.perm, plan.n
    for k in ks(plan):
        kept = kept_labels(plan, k)
        m = int(sum(sizes[s - 1] for s in kept))
        assert plan.schur_size(k) == m
        pos = np.sort(np.concatenate([np.arange(offs[s - 1], offs[s - 1] + sizes[s - 1]) for s in kept]))
        assert np.array_equal(pos, np.arange(n - m, n)), "the kept separators are the tail of the permuted order"
        dofs = plan.schur_dofs(k)
        assert dofs.dtype == np.int32 and np.array_equal(dofs, perm[n - m:])


@pytest.mark.parametrize("name", NAMES)
def test_records_cover_the_stored_lower_triangle_once(plans, name):
    plan = plans(name)
    sizes, offs = plan.sep_sizes.astype(np.int64), plan.sep_offsets.astype(np.int64)
    blocks = {(int(b[0]), int(b[1])): b for b in plan.blocks}
    for k in ks(plan):
        kept = set(kept_labels(plan, k))
        m = plan.schur_size(k)
        t0 = plan.n - m
        want = {}  # arena offset -> (row, column) of S, from the block table and the tile maps
        for (r, c), b in blocks.items():
            if r not in kept or c not in kept:
                continue
            ld, off = int(b[6]), int(b[7])
            tmap = plan.block_tile_map(r, c)
            for t, st in enumerate(tmap):
                if st < 0:
                    continue
                for i in range(16 * t, min(16 * t + 16, int(sizes[r - 1]))):
                    for j in range(int(sizes[c - 1]) if r != c else i + 1):
                        want[off + 16 * int(st) + i % 16 + j * ld] = (int(offs[r - 1]) - t0 + i, int(offs[c - 1]) - t0 + j)
        rec = plan.schur_list(k)
        assert rec.shape[1] == plan.SCHUR_RECORD
        got, count = {}, 0
        for off, ld, rows, cols, row0, col0, diag in rec:
            assert 0 < rows <= 16 and cols > 0 and diag in (0, 1)
            i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
            keep = (row0 + i >= col0 + j) if diag else np.ones_like(i, dtype=bool)
            if not diag:
                assert row0 >= col0 + cols, "an off-diagonal piece lies strictly under the diagonal"
            for a, R, Cc in zip((off + i + j * ld)[keep], (row0 + i)[keep], (col0 + j)[keep]):
                got[int(a)] = (int(R), int(Cc))
                count += 1
        assert count == len(got), "a position is covered twice"
        assert got == want
        assert all(0 <= a < plan.arena_doubles for a in got)
        assert all(0 <= c <= r < m for r, c in got.values())


@pytest.mark.parametrize("name", NAMES)
def test_schur_host_of_the_plain_fill_is_a_tt(plans, name):
    plan = plans(name)
    arena = plan.fill_host()
    D = plan.arena_to_dense(arena)
    A = np.tril(D) + np.tril(D, -1).T
    for k in ks(plan):
        m = plan.schur_size(k)
        t0 = plan.n - m
        S = plan.schur_host(k, arena)
        assert S.shape == (m, m)
        assert np.array_equal(S, A[t0:, t0:])
        # a wider leading dimension: the same numbers, the padding rows untouched
        S2 = plan.schur_host(k, arena, lds=m + 3)
        assert S2.shape == (m + 3, m) and np.array_equal(S2[:m], S) and np.isnan(S2[m:]).all()


def test_a_marked_arena_reads_back_through_the_records(plans):
    """schur_host on an arena whose every element is its own offset: each stored position of S shows the offset the records name, the rest is 0."""
    plan = plans("lapl_400x400")
    k = 3
    arena = np.arange(1, plan.arena_doubles + 1, dtype=np.float64)
    S = plan.schur_host(k, arena)
    m = plan.schur_size(k)
    want = np.zeros((m, m))
    for off, ld, rows, cols, row0, col0, diag in plan.schur_list(k):
        for i in range(rows):
            for j in range(cols):
                if diag and row0 + i < col0 + j:
                    continue
                want[row0 + i, col0 + j] = want[col0 + j, row0 + i] = off + i + j * ld + 1
    assert np.array_equal(S, want)
    assert (want == 0).any(), "lapl_400x400, k = 3 has unrelated separators and tiles without storage"


def test_out_of_range_arguments_are_refused(ca, plans):
    plan = plans("lapl_400x400")
    L = plan.L
    arena = plan.fill_host()
    for k in (0, -1, plan.levels, plan.levels + 3):
        assert L.cholamd_plan_schur_size(plan.h, k) == -4
        assert L.cholamd_plan_schur_dofs(plan.h, k, None) == -4
        assert L.cholamd_plan_schur_list(plan.h, k, 0, None) == -4
        with pytest.raises(ca.CholamdError):
            plan.schur_size(k)
        with pytest.raises(ca.CholamdError):
            plan.schur_host(k, arena)
    k = 2
    m = plan.schur_size(k)
    buf = np.full(m * m + 8, -7.0)
    for lds in (m - 1, 0, -5):
        assert L.cholamd_plan_schur_host(plan.h, k, arena.ctypes.data, buf.ctypes.data, lds) == -4
        assert (buf == -7.0).all()
    assert L.cholamd_plan_schur_host(plan.h, k, None, buf.ctypes.data, m) == -4
    assert L.cholamd_plan_schur_host(plan.h, k, arena.ctypes.data, None, m) == -4
    assert (buf == -7.0).all()
    assert "lds" in L.cholamd_last_error().decode() or "NULL" in L.cholamd_last_error().decode()
    # the largest allowed k is levels - 1
    assert plan.schur_size(plan.levels - 1) > plan.schur_size(plan.levels - 2)
    # cap smaller than the count: the count comes back, only cap records are written
    cnt = L.cholamd_plan_schur_list(plan.h, k, 0, None)
    out = np.full((cnt, plan.SCHUR_RECORD), -1, dtype=np.int64)
    assert L.cholamd_plan_schur_list(plan.h, k, 2, out.ctypes.data) == cnt
    assert (out[2:] == -1).all() and np.array_equal(out[:2], plan.schur_list(k)[:2])
