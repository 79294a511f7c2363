"""Host restatement of the deterministic streamed solve (cholamd_plan_solve_det_host, option solve_deterministic of the device): the step lists of both
sweeps walked over a host arena -- no device needed.

Inputs: the four fixtures and the synthetic trees tree_tiny, tree_single, tree_two, tree_over, tree_at, tree_skew.  The arena holds an independent
factor as in test_multiply_host -- the dense fp64 Cholesky factor of P A P^T on the stored positions of the lower triangle, NaN everywhere else (the
upper triangles of the diagonal blocks, padding rows, tiles without storage): a NaN in x means the walk read something that is not part of the factor.

Gates (none measured from the code under test):
  * x against the CPU oracle's x: the fixtures at 1e-10 max(1, |x|_max), the gate of the fixtures' host and GPU solve tests; the trees in
    SPD.forward_error at SPD.tol_forward() = C_FE (k + 1) u kappa, the gate of their GPU solve tests, against the oracle's x and the dense reference's.
  * which = 1 after which = 0 equals which = -1 bit for bit.
  * multiply_host(which)(solve_det_host(which)(b)) against b at tol_forward = C_FE (k + 1) u kappa (spd_inputs' constants, k and kappa of the input at
    hand), in measures that a symmetric diagonal scaling leaves alone: FORWARD, b a right-hand side: max |S^-1 (M y - b)| / max |S^-1 b|; BACKWARD, b
    white: max |M^T x - b| / max |b|.
  * the lists: in every step a permuted position has at most one owner, it is not solved yet and lies in the step's level (a lead step) or spans; no
    source of the step is owned in it; every source was solved by an earlier step; over a sweep every position is solved exactly once; every source lies
    on stored positions of the strictly lower triangle; the entries of the counts are those the lists and the spans' triangles add up to."""
import numpy as np
import pytest

import multiply_ref as mr
import tree_inputs
from conftest import CASES, case_paths
from spd_inputs import C_FE, U64

FWD, BWD = 0, 1
TREE_NAMES = ["tree_tiny", "tree_single", "tree_two", "tree_over", "tree_at", "tree_skew"]
NAMES = list(CASES) + TREE_NAMES
SPAN = 256


class Input:
    """plan, host arena (dense factor on the stored lower triangle, NaN elsewhere), b, the oracle's x and the measures of one input."""

    def __init__(self, name, tmp, golden):
        import cholesky_amd as ca
        from oracle import oracle as orc
        self.name = name
        if name in CASES:
            files = case_paths(name)
            self.plan = ca.Plan(*files[:3])
            g = golden(name)
            self.b, self.xo = np.asarray(g["b"], dtype=np.float64).ravel(), np.asarray(g["x"], dtype=np.float64).ravel()
            self.S = None
        else:
            self.S = tree_inputs.cached(tmp, name)
            self.plan = self.S.plan
            orc.use_own_kernels()
            O = orc.Oracle(self.S.mtx, self.S.ord, self.S.clust)
            O.factor()
            self.b, self.xo = self.S.rhs, O.solve(self.S.rhs)
        P = self.plan
        D = P.arena_to_dense(P.fill_host())
        self.PAP = np.tril(D) + np.tril(D, -1).T
        self.Ld = np.linalg.cholesky(self.PAP)
        self.arena = mr.arena_from_lower(P, self.Ld)
        self.perm = P.perm
        self.sp = np.sqrt(np.diag(self.PAP))                       # equilibration, permuted order
        self.s = np.empty(P.n)
        self.s[self.perm] = self.sp
        self.k = int((self.Ld != 0).sum(axis=1).max())
        self.kappa = self.S.kappa if self.S is not None else self._kappa()

    def _kappa(self, iters=60):
        """kappa_2 of the equilibrated matrix as SPD.equilibrated_condition computes it."""
        import scipy.linalg as sl
        Ae = self.PAP / self.sp[:, None] / self.sp[None, :]
        lmax = np.abs(Ae).sum(axis=1).max()
        Le = self.Ld / self.sp[:, None]
        v = np.random.default_rng(0).standard_normal(len(self.sp))
        mu = 0.0
        for _ in range(iters):
            v /= np.linalg.norm(v)
            y = sl.cho_solve((Le, True), v)
            mu = float(v @ y)
            v = y
        return lmax * mu

    def tol_forward(self):
        return C_FE * (self.k + 1) * U64 * self.kappa


_INPUTS = {}


@pytest.fixture
def inputs(tmp_path_factory, golden):
    def get(name):
        if name not in _INPUTS:
            _INPUTS[name] = Input(name, tmp_path_factory, golden)
        return _INPUTS[name]
    return get


@pytest.fixture(autouse=True)
def environment(monkeypatch):
    for v in ("CHOLAMD_COMPACT", "CHOLAMD_SOLVE_NO_BAND"):
        monkeypatch.delenv(v, raising=False)


@pytest.mark.parametrize("name", NAMES)
def test_host_solve_matches_the_oracle(name, inputs):
    I = inputs(name)
    P = I.plan
    assert np.isnan(I.arena).any() or P.n == 1, "the upper triangles and the padding hold NaN"
    x = P.solve_det_host(I.arena, -1, I.b)
    assert np.isfinite(x).all()
    if I.S is None:
        err, gate = float(np.abs(x - I.xo).max()), 1e-10 * max(1.0, float(np.abs(I.xo).max()))
        print(f"{name}: |x - x_oracle| = {err:.3e} (gate {gate:.3e})")
        assert err <= gate
    else:
        gate = I.S.tol_forward()
        eo, er = I.S.forward_error(x, I.xo), I.S.forward_error(x)
        print(f"{name}: forward error against the oracle {eo:.3e}, against the dense reference {er:.3e} (gate {gate:.3e})")
        assert eo <= gate and er <= gate
    # the halves compose to the solve, bit for bit; in place gives the same bits
    y = P.solve_det_host(I.arena, FWD, I.b)
    assert np.array_equal(P.solve_det_host(I.arena, BWD, y), x)
    w = I.b.copy()
    assert P.L.cholamd_plan_solve_det_host(P.h, I.arena.ctypes.data, -1, w.ctypes.data, w.ctypes.data) == 0
    assert np.array_equal(w, x)


@pytest.mark.parametrize("name", NAMES)
def test_product_undoes_the_half_solve(name, inputs):
    I = inputs(name)
    P = I.plan
    tol = I.tol_forward()
    w = np.random.default_rng(31).standard_normal(P.n)
    b = I.s * w                                                    # a right-hand side
    y = P.solve_det_host(I.arena, FWD, b)
    e = float(np.abs((P.multiply_host(I.arena, FWD, y) - b) / I.s).max() / np.abs(w).max())
    print(f"{name} FORWARD: {e:.3e} (tol {tol:.3e})")
    assert e <= tol
    x = P.solve_det_host(I.arena, BWD, w)                          # white input
    e = float(np.abs(P.multiply_host(I.arena, BWD, x) - w).max() / np.abs(w).max())
    print(f"{name} BACKWARD: {e:.3e} (tol {tol:.3e})")
    assert e <= tol


def _level_seps(P, level):
    """(first position, columns) of the separators of a tree level."""
    tree, size, off = P.tree, P.sep_sizes, P.sep_offsets
    return [(int(off[tree[h - 1] - 1]), int(size[tree[h - 1] - 1])) for h in range(1 << level, min(1 << (level + 1), P.nsep + 1))]


@pytest.mark.parametrize("name", NAMES)
def test_list_invariants(name, inputs):
    I = inputs(name)
    P = I.plan
    img = mr.index_image(P)
    stored = np.zeros(P.arena_doubles + 1, dtype=bool)             # arena offsets (+ 1) of the strictly lower triangle
    stored[np.tril(img, -1).ravel()] = True
    stored[0] = False
    counts = P.solve_det_counts()
    for which, tag in ((FWD, "forward"), (BWD, "backward")):
        steps, items, srcs = P.solve_det_lists(which)
        c = counts[tag]
        assert (len(steps), len(items), len(srcs)) == (c["steps"], c["items"], c["sources"])
        levels = steps[:, 0]
        assert (np.diff(levels) <= 0).all() if which == FWD else (np.diff(levels) >= 0).all()
        solved = np.zeros(P.n, dtype=np.int64)
        done = np.zeros(P.n, dtype=bool)
        at, read = 0, 0
        for level, col0, i0, i1 in steps:
            assert i0 == at and i1 >= i0 and (col0 == -1 or (col0 >= 0 and col0 % SPAN == 0))
            at = i1
            owned = np.zeros(P.n, dtype=np.int64)
            for y_off, nv, s0, s1 in items[i0:i1]:
                assert 1 <= nv <= 16 and s1 > s0
                owned[y_off:y_off + nv] += 1
            assert owned.max(initial=0) <= 1, "a position with two owners in one step"
            for y_off, nv, s0, s1 in items[i0:i1]:
                for a_off, ld, ln, z_off, tri in srcs[s0:s1]:
                    assert ln >= 1 and done[z_off:z_off + ln].all(), "a source that is not solved yet"
                    assert not owned[z_off:z_off + ln].any(), "a source that is owned in its own step"
                    lines, ks = np.arange(nv), np.arange(ln)
                    idx = a_off + (lines[:, None] + ks[None, :] * ld if which == FWD else ks[None, :] + lines[:, None] * ld)
                    assert stored[idx + 1].all(), "a source off the stored lower triangle"
                    read += idx.size
            span = np.zeros(P.n, dtype=bool)
            if col0 < 0:                                           # a level's lead step: it owns unsolved positions of its level and solves nothing
                lvl = np.zeros(P.n, dtype=bool)
                for x0, n in _level_seps(P, int(level)):
                    lvl[x0:x0 + n] = True
                assert not (owned.astype(bool) & (~lvl | done)).any(), "a lead item outside its level, or on a solved position"
                continue
            for x0, n in _level_seps(P, int(level)):
                lo, hi = min(n, int(col0)), min(n, int(col0) + SPAN)
                span[x0 + lo:x0 + hi] = True
                read += (hi - lo) * (hi - lo + 1) // 2
            assert span.any() and not (owned.astype(bool) & (~span | done)).any(), "an item outside its step's spans, or on a solved position"
            solved += span
            done |= span
        assert at == len(items) and (solved == 1).all(), "every position is solved exactly once"
        assert read == c["entries"]
    assert P.L.cholamd_plan_solve_det_counts(P.h, None) == -4 and P.L.cholamd_plan_solve_det_counts(None, None) == -4


@pytest.mark.parametrize("name", ["lapl_400x400", "tree_over", "tree_skew", "tree_single"])
def test_nan_outside_the_factor_does_not_reach_x(name, inputs):
    """Upper triangles, padding rows and tiles without storage as zeros and as NaN: the same bits."""
    I = inputs(name)
    P = I.plan
    clean = mr.arena_from_lower(P, I.Ld, fill=0.0)
    assert np.isnan(I.arena).any() and not np.isnan(clean).any()
    for which in (FWD, BWD, -1):
        a, b = P.solve_det_host(clean, which, I.b), P.solve_det_host(I.arena, which, I.b)
        assert np.isfinite(b).all() and np.array_equal(a, b), (name, which)


def test_bad_arguments_are_refused(inputs):
    I = inputs("lapl_9x9")
    P = I.plan
    b, x = np.ones(P.n), np.full(P.n, -7.0)
    f = P.L.cholamd_plan_solve_det_host
    for which in (2, -2):
        assert f(P.h, I.arena.ctypes.data, which, b.ctypes.data, x.ctypes.data) == -4
        assert "which" in P.L.cholamd_last_error().decode()
    assert f(P.h, None, 0, b.ctypes.data, x.ctypes.data) == -4
    assert f(P.h, I.arena.ctypes.data, 0, None, x.ctypes.data) == -4
    assert f(P.h, I.arena.ctypes.data, 0, b.ctypes.data, None) == -4
    assert f(None, I.arena.ctypes.data, 0, b.ctypes.data, x.ctypes.data) == -4
    assert (x == -7.0).all()


def test_the_device_knows_the_option():
    """Where a GPU exists the device object accepts the option; elsewhere the symbols of the host side are all there is to check."""
    import cholesky_amd as ca
    L = ca.load()
    for sym in ("cholamd_plan_solve_det_host", "cholamd_plan_solve_det_counts", "cholamd_plan_solve_det_lists", "cholamd_device_set_option"):
        assert hasattr(L, sym)
    plan = ca.Plan(*case_paths("lapl_9x9")[:3])
    c = plan.solve_det_counts()
    assert c["forward"]["steps"] == c["backward"]["steps"] >= 2 * plan.levels
    if L.cholamd_device_count() > 0:
        dev = ca.Device(plan, 0)
        dev.set_option("solve_deterministic", 1)
        dev.set_option("solve_deterministic", 0)
