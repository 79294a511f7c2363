"""Host restatement of the block Schur condense / expand (cholamd_plan_schur_condense_host_nrhs / _expand_host_nrhs, device option schur_deterministic):
the deterministic step lists CUT at k kept levels walked over a host arena on chunks of 32 columns -- no device needed.

The arena: the eliminated part factored, the kept part holding S, from dense numpy on A = P A P^T (I = [0, t0), T = [t0, n)):
L_I = chol(A_II), L_TI = A_TI L_I^-T, S = A_TT - L_TI L_TI^T; [[L_I, 0], [L_TI, tril(S)]] goes to the stored positions of the lower triangle
(multiply_ref.arena_from_lower), NaN everywhere else.

Gates (none measured from the code under test), per column: |G - g_ref|_max <= 1e-12 |g_ref|_max with g_ref = b_T - A_TI solve(A_II, b_I); X (expanded
from XT = solve(S, G)) against the dense solve at 1e-10 |x_ref|_max and ||b - A x|| <= 1e-10 ||b||: the gates of tests/test_gpu_schur.py.  Everything
else is bit for bit."""
import numpy as np
import pytest

import multiply_ref as mr
import tree_inputs
from conftest import CASES, case_paths

SHAPES = [("lapl_25x25", 2), ("lapl_400x400", 3), ("tree_tiny", 1), ("tree_tiny", 3), ("tree_over", 1), ("tree_over", 2)]
IDS = [f"{c}-k{k}" for c, k in SHAPES]
NRHS = 33                                                            # two chunks, the second of one column
_BASE, _CUT = {}, {}


class Base:
    """plan, A = P A P^T (permuted, dense) and a block of right-hand sides (original dof order) of one input."""

    def __init__(self, name, tmp):
        import cholesky_amd as ca
        if name in CASES:
            files = case_paths(name)
            self.plan = ca.Plan(*files[:3])
            b = np.asarray(ca.plan.read_vector(files[3], self.plan.n), dtype=np.float64)
            D = self.plan.arena_to_dense(self.plan.fill_host())
            self.A = np.tril(D) + np.tril(D, -1).T
        else:
            S = tree_inputs.cached(tmp, name)
            self.plan, b, self.A = S.plan, np.asarray(S.rhs, dtype=np.float64), np.asarray(S.PAP, dtype=np.float64)
        P = self.plan
        s = np.empty(P.n)
        s[P.perm] = np.sqrt(np.diag(self.A))                         # the equilibration, as the solve tests scale their right-hand sides
        self.B = s[:, None] * np.random.default_rng(91).standard_normal((P.n, NRHS))
        self.B[:, 0] = b
        self.B.setflags(write=False)


class Cut:
    """The partially factored arena of (input, k), its references and the host results on the whole block, computed once."""

    def __init__(self, base, k):
        import scipy.linalg as sl
        P, A = base.plan, base.A
        self.base, self.k, self.plan = base, k, P
        self.m = P.schur_size(k)
        self.t0 = t0 = P.n - self.m
        LI = np.linalg.cholesky(A[:t0, :t0])
        LTI = sl.solve_triangular(LI, A[:t0, t0:], lower=True).T
        self.S = A[t0:, t0:] - LTI @ LTI.T
        Lfull = np.zeros_like(A)
        Lfull[:t0, :t0], Lfull[t0:, :t0], Lfull[t0:, t0:] = LI, LTI, np.tril(self.S)
        self.arena = mr.arena_from_lower(P, Lfull)
        self.arena.setflags(write=False)
        Bp = base.B[P.perm]
        self.Gref = Bp[t0:] - A[t0:, :t0] @ np.linalg.solve(A[:t0, :t0], Bp[:t0])
        Xp = np.linalg.solve(A, Bp)
        self.Xref = np.empty_like(Xp)
        self.Xref[P.perm] = Xp
        self.W, self.G = P.schur_condense_host_nrhs(k, self.arena, base.B, ldb=P.n + 3, ldw=P.n + 1, ldg=self.m + 2)
        self.XT = np.linalg.solve(self.S, self.G)
        self.X = P.schur_expand_host_nrhs(k, self.arena, self.W, self.XT, ldw=P.n + 2, ldxt=self.m + 1, ldx=P.n + 3)
        for a in (self.W, self.G, self.XT, self.X):
            a.setflags(write=False)


@pytest.fixture
def cut(tmp_path_factory):
    def get(name, k):
        if name not in _BASE:
            _BASE[name] = Base(name, tmp_path_factory)
        if (name, k) not in _CUT:
            _CUT[name, k] = Cut(_BASE[name], k)
        return _CUT[name, k]
    return get


@pytest.fixture(autouse=True)
def environment(monkeypatch):
    for v in ("CHOLAMD_COMPACT", "CHOLAMD_SOLVE_NO_BAND"):
        monkeypatch.delenv(v, raising=False)


@pytest.mark.parametrize("name,k", SHAPES, ids=IDS)
def test_every_column_matches_the_dense_reference(name, k, cut):
    C = cut(name, k)
    P, A, B = C.plan, C.base.A, C.base.B
    assert np.isnan(C.arena).any(), "the upper triangles and the padding hold NaN"
    assert C.W.shape == (P.n, NRHS) and C.G.shape == (C.m, NRHS) and C.X.shape == (P.n, NRHS)
    assert np.isfinite(C.W).all() and np.isfinite(C.X).all()
    assert np.array_equal(C.W[C.t0:], C.G), "the tail of W is G"
    worst = [0.0, 0.0, 0.0]
    for j in range(NRHS):
        gerr = float(np.abs(C.G[:, j] - C.Gref[:, j]).max() / np.abs(C.Gref[:, j]).max())
        xerr = float(np.abs(C.X[:, j] - C.Xref[:, j]).max() / np.abs(C.Xref[:, j]).max())
        bp, xp = B[P.perm, j], C.X[P.perm, j]
        res = float(np.linalg.norm(bp - A @ xp) / np.linalg.norm(bp))
        worst = [max(a, b) for a, b in zip(worst, (gerr, xerr, res))]
    print(f"{name} k = {k}: worst column |G - g_ref| / |g_ref| = {worst[0]:.3e} (gate 1e-12), |X - x_ref| / |x_ref| = {worst[1]:.3e} (gate 1e-10), "
          f"residual = {worst[2]:.3e} (gate 1e-10)")
    assert worst[0] <= 1e-12 and worst[1] <= 1e-10 and worst[2] <= 1e-10


@pytest.mark.parametrize("name,k", SHAPES, ids=IDS)
def test_columns_are_independent_and_repeatable(name, k, cut):
    C = cut(name, k)
    P, B = C.plan, C.base.B
    W2, G2 = P.schur_condense_host_nrhs(k, C.arena, B)
    assert np.array_equal(W2, C.W) and np.array_equal(G2, C.G), "two calls, other leading dimensions: the same bits"
    assert np.array_equal(P.schur_expand_host_nrhs(k, C.arena, C.W, C.XT), C.X)
    for j in (0, 17, 32):
        w, g = P.schur_condense_host_nrhs(k, C.arena, B[:, j:j + 1])
        assert np.array_equal(w[:, 0], C.W[:, j]) and np.array_equal(g[:, 0], C.G[:, j]), (j, "alone")
        assert np.array_equal(P.schur_expand_host_nrhs(k, C.arena, C.W[:, j:j + 1], C.XT[:, j:j + 1])[:, 0], C.X[:, j]), (j, "alone")
    order = np.roll(np.arange(NRHS), 13)                             # chunks and half-tiles change
    Wp, Gp = P.schur_condense_host_nrhs(k, C.arena, B[:, order])
    assert np.array_equal(Wp, C.W[:, order]) and np.array_equal(Gp, C.G[:, order])
    assert np.array_equal(P.schur_expand_host_nrhs(k, C.arena, C.W[:, order], C.XT[:, order]), C.X[:, order])
    Bn = B.copy()
    Bn[:, 7] = np.nan
    Bn[3, 32] = np.nan
    keep = [j for j in range(NRHS) if j not in (7, 32)]
    Wn, Gn = P.schur_condense_host_nrhs(k, C.arena, Bn)
    assert np.isnan(Wn[:, 7]).any() and np.array_equal(Wn[:, keep], C.W[:, keep]) and np.array_equal(Gn[:, keep], C.G[:, keep])
    Wn, Tn = C.W.copy(), C.XT.copy()
    Wn[:, 7] = np.nan
    Tn[0, 32] = np.nan
    Xn = P.schur_expand_host_nrhs(k, C.arena, Wn, Tn)
    assert np.isnan(Xn[:, 7]).any() and np.isnan(Xn[:, 32]).any() and np.array_equal(Xn[:, keep], C.X[:, keep])


def piece_offsets(plan, k):
    """Every arena offset a piece of schur_list(k) covers (the whole 16-row tile of a diagonal block's piece, its upper part included)."""
    offs = [(off + np.arange(rows)[:, None] + np.arange(cols)[None, :] * ld).ravel() for off, ld, rows, cols, _, _, _ in plan.schur_list(k)]
    return np.unique(np.concatenate(offs))


@pytest.mark.parametrize("name,k", SHAPES, ids=IDS)
def test_s_is_never_read(name, k, cut):
    """Contract (c): NaN over every element that schur_list(k) covers changes no bit of W, G, X."""
    C = cut(name, k)
    P = C.plan
    bad = C.arena.copy()
    cover = piece_offsets(P, k)
    assert np.isfinite(bad[cover]).any()
    bad[cover] = np.nan
    W, G = P.schur_condense_host_nrhs(k, bad, C.base.B)
    assert np.array_equal(W, C.W) and np.array_equal(G, C.G)
    assert np.array_equal(P.schur_expand_host_nrhs(k, bad, C.W, C.XT), C.X)


@pytest.mark.parametrize("name,k", SHAPES, ids=IDS)
def test_the_cut_lists_from_outside(name, k, cut):
    C = cut(name, k)
    P, t0, n = C.plan, C.t0, C.plan.n
    cover = piece_offsets(P, k)
    counts = P.schur_det_counts(k)
    levels_of = np.empty(n, dtype=np.int64)                          # tree level per permuted position
    offs, sizes = P.sep_offsets, P.sep_sizes
    for h in range(1, P.nsep + 1):
        lbl = int(P.tree[h - 1])
        levels_of[offs[lbl - 1]:offs[lbl - 1] + sizes[lbl - 1]] = h.bit_length() - 1
    for which, key in ((0, "forward"), (1, "backward")):
        steps, items, srcs = P.schur_det_lists(k, which)
        assert (len(steps), len(items), len(srcs)) == (counts[key]["steps"], counts[key]["items"], counts[key]["sources"])
        lead = [t for t in range(len(steps)) if steps[t, 0] == -1]
        assert lead == ([len(steps) - 1] if which == 0 else []), "one kept lead step, the last of the forward list"
        solved = np.zeros(n, dtype=np.int64)
        owned = np.zeros(n, dtype=np.int64)
        entries = 0
        for lvl, col0, i0, i1 in steps:
            assert lvl == -1 or lvl >= k
            for y_off, nv, s0, s1 in items[i0:i1]:
                assert 1 <= nv <= 16 and s1 > s0
                if lvl == -1:
                    assert y_off >= t0 and col0 == -1
                    owned[y_off:y_off + nv] += 1
                else:
                    assert y_off + nv <= t0 and (levels_of[y_off:y_off + nv] == lvl).all()
                for a_off, ld, ln, z_off, tri in srcs[s0:s1]:
                    entries += nv * ln
                    if lvl == -1:
                        assert z_off + ln <= t0, "a kept-lead source reads under the cut only"
                    if which == 0:
                        assert z_off + ln <= t0
                        touched = a_off + np.arange(nv)[:, None] + np.arange(ln)[None, :] * ld
                    else:
                        touched = a_off + np.arange(ln)[:, None] + np.arange(nv)[None, :] * ld
                    assert touched.min() >= 0 and touched.max() < P.arena_doubles
                    assert not np.isin(touched.ravel(), cover).any(), "a source offset falls in a schur_list piece"
            if col0 >= 0:
                for h in range(1 << lvl, min(1 << (lvl + 1), P.nsep + 1)):
                    lbl = int(P.tree[h - 1])
                    lo, hi = offs[lbl - 1] + col0, offs[lbl - 1] + min(sizes[lbl - 1], col0 + 256)
                    if hi > lo:
                        solved[lo:hi] += 1
                        entries += (hi - lo) * (hi - lo + 1) // 2
        assert (solved[:t0] == 1).all() and (solved[t0:] == 0).all(), "every position under the cut is solved once, none above it"
        assert (owned <= 1).all()
        assert entries == counts[key]["entries"]


def test_bad_arguments_are_refused(cut):
    C = cut("lapl_25x25", 2)
    P, k, n, m, c = C.plan, 2, C.plan.n, C.m, 3
    SENT = -7.0
    B, W, G, X, XT = np.ones((c, n)), np.full((c, n), SENT), np.full((c, m), SENT), np.full((c, n), SENT), np.ones((c, m))
    fc, fe = P.L.cholamd_plan_schur_condense_host_nrhs, P.L.cholamd_plan_schur_expand_host_nrhs
    ar, b, w, g, x, xt = (a.ctypes.data for a in (C.arena, B, W, G, X, XT))
    for bad in (0, -1, P.levels, P.levels + 2):
        assert fc(P.h, bad, ar, b, n, w, n, g, m, c) == -4 and fe(P.h, bad, ar, w, n, xt, m, x, n, c) == -4
        assert P.L.cholamd_plan_schur_det_counts(P.h, bad, np.zeros(8, dtype=np.int64).ctypes.data) == -4
    assert fc(None, k, ar, b, n, w, n, g, m, c) == -4 and fe(None, k, ar, w, n, xt, m, x, n, c) == -4
    for args in ((None, b, n, w, n, g, m), (ar, None, n, w, n, g, m), (ar, b, n, None, n, g, m), (ar, b, n, w, n, None, m),
                 (ar, b, n - 1, w, n, g, m), (ar, b, n, w, n - 1, g, m), (ar, b, n, w, n, g, m - 1)):
        assert fc(P.h, k, *args, c) == -4, args
    for args in ((None, w, n, xt, m, x, n), (ar, None, n, xt, m, x, n), (ar, w, n, None, m, x, n), (ar, w, n, xt, m, None, n),
                 (ar, w, n - 1, xt, m, x, n), (ar, w, n, xt, m - 1, x, n), (ar, w, n, xt, m, x, n - 1)):
        assert fe(P.h, k, *args, c) == -4, args
    assert fc(P.h, k, ar, b, n, w, n, g, m, -1) == -4 and fe(P.h, k, ar, w, n, xt, m, x, n, -1) == -4
    assert (W == SENT).all() and (G == SENT).all() and (X == SENT).all()
    # nrhs = 0: accepted, nothing is read or written
    assert fc(P.h, k, None, None, n, None, n, None, m, 0) == 0 and fe(P.h, k, None, None, n, None, m, None, n, 0) == 0
    assert (W == SENT).all() and (G == SENT).all() and (X == SENT).all()
    with pytest.raises(Exception):
        P.schur_det_lists(k, 2)


def test_the_library_has_the_entry_points():
    import cholesky_amd as ca
    L = ca.load()
    for f in ("cholamd_plan_schur_condense_host_nrhs", "cholamd_plan_schur_expand_host_nrhs", "cholamd_plan_schur_det_counts", "cholamd_plan_schur_det_lists",
              "cholamd_schur_condense_nrhs", "cholamd_schur_condense_nrhs_f32", "cholamd_schur_expand_nrhs", "cholamd_schur_expand_nrhs_f32"):
        assert hasattr(L, f)
