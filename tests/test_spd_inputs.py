"""CPU tests of the general SPD inputs (tests/spd_inputs.py): the builder's matrices, the host fill, the CPU oracle, the solve's skipped
entries and the program launch's self-check on patterns and values that are not a grid Laplacian's."""
import numpy as np
import pytest

import spd_inputs as si

# the host-side inputs: every pattern family, a scaled one and the ragged grid (the 5832-column 27-point input is the GPU file's)
HOST = ["lapl_400x400", "lapl_3375_scaled", "g12_full", "g16_subset", "g20_2d", "g7_ragged"]


@pytest.fixture(scope="module")
def spd(tmp_path_factory):
    return lambda name: si.cached(tmp_path_factory, name)


@pytest.mark.parametrize("name", HOST)
def test_builder_gives_spd_matrices_the_host_fill_reproduces(name, spd):
    S = spd(name)
    assert S.plan.dropped == 0
    assert np.all(np.isfinite(S.Ld)) and np.all(np.diag(S.Ld) > 0)      # numpy's dense Cholesky succeeded: SPD
    assert np.array_equal(S.A, S.A.T)
    off = S.A[~np.eye(S.n, dtype=bool)]
    if name != "lapl_3375_scaled":
        assert (off > 0).any() and (off < 0).any()                      # mixed signs, unlike every Laplacian
    # the values round-trip through the file and land where P A P^T has them, entry for entry
    H = S.plan.arena_to_dense(S.plan.fill_host())
    assert np.array_equal(np.tril(H), np.tril(S.PAP))
    assert len(np.unique(np.abs(off[off != 0]))) > S.n                  # values differ from entry to entry


@pytest.mark.parametrize("name", HOST)
def test_oracle_factor_matches_dense_cholesky(name, spd):
    S = spd(name)
    assert S.row_error(S.Lo) <= S.tol_factor()
    assert S.reconstruction(S.Lo) <= S.tol_reconstruction()
    # the oracle's factor has no entry outside dense numpy's structure
    assert not S.Lo[S.Ld == 0].any()


def test_builder_options_do_what_they_say(tmp_path):
    """27-point / subset patterns, negative signs, scaling: the nnz and the signs of the written matrix."""
    full = si.SPD(tmp_path, (6, 5, 4, 2, 8), 1, pattern="full", signs="negative", oracle=False, name="full")
    r, c = si._stencil_edges(6, 5, 4)
    assert len(full.val) == full.n + len(r)
    assert (full.val[full.n:] < 0).all()
    sub = si.SPD(tmp_path, (6, 5, 4, 2, 8), 1, pattern="subset", p=0.4, oracle=False, name="sub")
    assert 0.3 * len(r) < len(sub.val) - sub.n < 0.5 * len(r)
    flat = si.SPD(tmp_path, (7, 6, 1, 2, 8), 1, pattern="full", oracle=False, name="flat")
    assert len(flat.val) - flat.n == 4 * 7 * 6 - 3 * 7 - 3 * 6 + 2   # 9-point in 2-D: 4 edge directions
    sc = si.SPD(tmp_path, (6, 5, 4, 2, 8), 1, pattern="full", scale=3.0, oracle=False, name="sc")
    assert np.diag(sc.A).max() / np.diag(sc.A).min() > 1e4
    # the equilibrated condition number tracks sigma: a negative-sign stencil plus sigma I has lambda_min = sigma exactly
    nearly = si.SPD(tmp_path, (6, 5, 4, 2, 8), 1, pattern="full", signs="negative", sigma=1e-6, oracle=False, name="nearly")
    assert nearly.kappa > 1e6 * full.kappa / 10


@pytest.mark.parametrize("name", HOST)
def test_what_the_solve_skips_is_zero_in_the_factor_of_general_inputs(name, spd):
    """The zero claims of cholamd_plan_solve_skips (leaf bands, c_lo) on 27-point, 9-point, random-subset and mixed-sign inputs: exactly zero in
    the oracle's factor, and zero in dense numpy's factor (no cancellation makes them zero by accident: numpy fills every structural non-zero)."""
    S = spd(name)
    P = S.plan
    skipped = 0
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
                    skipped += int((i - j > band).sum())
            for x_off, m, y_off, n, c_lo in runs:
                assert 0 <= c_lo <= n and c_lo % 16 == 0
                assert not Lf[x_off:x_off + m, y_off:y_off + c_lo].any()
                skipped += m * c_lo
    if name != "g7_ragged":
        assert skipped > 0


@pytest.mark.parametrize("name", HOST)
def test_program_launch_check_on_general_inputs(name, spd):
    """The one-launch program's host self-check on the new plans: live with and without followers at 256, 32 and 4 resident workgroups."""
    P = spd(name).plan
    for follow in (1, 0):
        for workers in (256, 32, 4):
            P.program_check(follow, workers)


@pytest.mark.parametrize("name", ["lapl_400x400", "g16_subset", "g7_ragged"])
def test_sparse_arena_reader_equals_the_dense_one(name, spd):
    """spd_inputs.arena_to_sparse (block table + tile maps, no dense copy) reads the host fill as tril(arena_to_dense) does, and that is
    tril(P A P^T) built from the matrix file."""
    S = spd(name)
    host = S.plan.fill_host()
    Ls = si.arena_to_sparse(S.plan, host)
    assert np.array_equal(Ls.toarray(), np.tril(S.plan.arena_to_dense(host)))
    assert np.array_equal(Ls.toarray(), np.tril(S.PAP))


def test_host_fill_of_leaves_wider_than_4096_columns(tmp_path):
    """Problem(20, 20, 25, 2, 64) with random values (the GPU file factors it): two leaves of 4 800 columns; without a dense copy of anything,
    the host fill read back through the sparse reader is tril(P A P^T) entry for entry."""
    import scipy.sparse as sp
    S = si.SPD(tmp_path, (20, 20, 25, 2, 64), 21, pattern="own", oracle=False, dense=False, name="wide")
    assert S.A is None and S.PAP is None
    assert max(S.plan.sep_sizes) == 4800
    got = si.arena_to_sparse(S.plan, S.plan.fill_host())
    want = sp.tril(S.permuted_sparse()).tocsr()
    assert got.nnz == want.nnz and (got != want).nnz == 0
