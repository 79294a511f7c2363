"""Host side of the gradients with respect to the value array (cholamd_plan_values_grad_pairs_host, cholamd_plan_values_grad_logdet_host,
cholamd_plan_duplicate_entries) -- no device needed.  The device kernels are held to these restatements bit for bit (test_gpu_values_grad.py).

Definition (include/cholamd.h): A(v) = sum_k v_k E_k, E_k = e_i e_j^T + e_j e_i^T off the diagonal (m_k = 2), e_i e_i^T on it (m_k = 1), (i, j) entry k
of plan.entries().  Pair sum s_k = sum_c p_c^T E_k q_c; log-det term t_k = tr(A^-1 E_k) = m_k (A^-1)(i, j); zero for entries outside the pattern.

Bounds.  The pair sum is a dot product of 2 nrhs terms (nrhs on the diagonal) accumulated by fma and scaled once: against the same sum in long double
|g_k - ref_k| <= (2 nrhs + 1) u sum|terms|, u = 2^-53 (Higham, Thm 3.1 with gamma_n ~ n u).  The log-det terms carry selinv_ref's bound
C_SEL (k + 1) u r_i r_j in the equilibrated matrix, as the selected inverse they are read from.  The analytic formulas themselves are checked against
central differences of numpy's dense solve and slogdet: a step h = 1e-5 |v_k| leaves a truncation term O(h^2) = 1e-10 and a rounding term
u / h = 1e-11 relative to the size of the loss's derivatives, four orders below the gate 1e-6 (of the largest derivative)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import selinv_ref as sr
import spd_inputs as si

U = si.U64
INPUTS = ["lapl_9x9", "lapl_25x25", "g7_ragged", "tree_tiny"]
NRHS = [1, 2, 31, 32, 33, 70]

SIGNATURES = {
    "cholamd_values_grad_pairs": ["cholamd_device *", "const double *", "int64_t", "const double *", "int64_t", "int", "double", "double", "double *", "int64_t", "void *"],
    "cholamd_values_grad_logdet": ["cholamd_device *", "const double *", "double", "double", "double *", "int64_t", "void *"],
    "cholamd_plan_values_grad_pairs_host": ["const cholamd_plan *", "const double *", "int64_t", "const double *", "int64_t", "int", "double", "double", "double *", "int64_t"],
    "cholamd_plan_values_grad_logdet_host": ["const cholamd_plan *", "const double *", "double", "double", "double *", "int64_t"],
}


@pytest.fixture(scope="module")
def spd(tmp_path_factory):
    return lambda name: si.cached(tmp_path_factory, name)


def pair_reference(row, col, P, Q, inpat=None):
    """(s_k in long double rounded to fp64, sum of the magnitudes of its terms) for every entry; zero where `inpat` is False."""
    Pl, Ql = P.astype(np.longdouble), Q.astype(np.longdouble)
    t1 = Pl[row] * Ql[col]
    t2 = np.where((row != col)[:, None], Pl[col] * Ql[row], 0)
    s, mag = (t1 + t2).sum(axis=1), (np.abs(t1) + np.abs(t2)).sum(axis=1)
    if inpat is not None:
        s, mag = np.where(inpat, s, 0), np.where(inpat, mag, 0)
    return s, mag


def in_pattern(plan):
    m = np.zeros(plan.nz, dtype=bool)
    m[plan.value_map()] = True
    return m


@pytest.mark.parametrize("name", INPUTS)
def test_pair_sums_against_long_double(name, spd):
    S = spd(name)
    plan = S.plan
    assert plan.nz == {"lapl_9x9": 21, "lapl_25x25": 65}.get(name, plan.nz)
    row, col = plan.entries()
    rng = np.random.default_rng(7)
    worst = 0.0
    for k in NRHS:
        P, Q = rng.standard_normal((S.n, k)), rng.standard_normal((S.n, k)) * 10.0 ** rng.uniform(-3, 3, (S.n, 1))
        for Qx, ldp, ldq in ((Q, None, None), (Q, S.n + 3, S.n + 7), (P, S.n + 1, S.n + 1)):
            g = plan.values_grad_pairs_host(P, Qx, ldp=ldp, ldq=ldq)
            ref, mag = pair_reference(row, col, P, Qx)
            err = np.abs(g.astype(np.longdouble) - ref)
            assert np.isfinite(g).all()
            assert (err <= (2 * k + 1) * U * mag).all(), (name, k, float((err / np.maximum(mag, 1e-300)).max() / U))
            worst = max(worst, float((err / np.maximum(mag * U, 1e-300)).max() / (2 * k + 1)))
    print(f"pair sums {name}: nz = {plan.nz}, largest error / bound = {worst:.3g}")


def test_alpha_and_beta(spd):
    S = spd("lapl_25x25")
    plan = S.plan
    rng = np.random.default_rng(8)
    P, Q = rng.standard_normal((S.n, 5)), rng.standard_normal((S.n, 5))
    s = plan.values_grad_pairs_host(P, Q, 1.0, 0.0, g=np.full(plan.nz, np.nan))          # beta == 0: g is not read
    assert np.isfinite(s).all()
    assert np.array_equal(plan.values_grad_pairs_host(P, Q, -1.0, 0.0), -s)
    g0 = rng.standard_normal(plan.nz)
    got = plan.values_grad_pairs_host(P, Q, 0.5, 2.0, g=g0)
    want = np.array([float(np.longdouble(0.5) * np.longdouble(a) + np.longdouble(2.0 * b)) for a, b in zip(s, g0)])    # one rounding: the fma
    assert np.array_equal(got, want)
    assert np.array_equal(plan.values_grad_pairs_host(P, Q, 0.0, 1.0, g=g0), g0)


def _with_explicit_zero(tmp_path):
    """test_gpu_selinv's construction: a subset stencil plus one explicit zero at a free position; returns (S, index of that entry)."""
    import cholesky_amd as ca
    S = si.SPD(str(tmp_path), (7, 5, 3, 3, 4), 11, pattern="subset", p=0.5, name="sub")
    free = np.argwhere(np.tril(S.A == 0, -1))
    i, j = (int(v) for v in free[len(free) // 2])
    row, col, val = np.append(S.row, i), np.append(S.col, j), np.append(S.val, 0.0)
    S.mtx = os.path.join(str(tmp_path), "sub_zero.mtx")
    si.write_mtx(S.mtx, S.n, row, col, val)
    S.plan = ca.Plan(S.mtx, S.ord, S.clust)
    assert S.plan.nz == len(val) and S.plan.nnz_a == len(val) - 1 and np.array_equal(S.plan.perm, S.perm)
    r, c = S.plan.entries()
    return S, int(np.nonzero((r == i) & (c == j))[0][0])


def test_entry_outside_the_pattern_gets_beta_g(tmp_path):
    S, k = _with_explicit_zero(tmp_path)
    plan = S.plan
    assert plan.duplicate_entries == 0 and not in_pattern(plan)[k]
    rng = np.random.default_rng(9)
    P, Q = rng.standard_normal((S.n, 3)), rng.standard_normal((S.n, 3))
    Za = rng.standard_normal(plan.arena_doubles)
    g0 = rng.standard_normal(plan.nz)
    for fn in (lambda a, b, g: plan.values_grad_pairs_host(P, Q, a, b, g=g), lambda a, b, g: plan.values_grad_logdet_host(Za, a, b, g=g)):
        assert fn(1.0, 0.0, np.full(plan.nz, np.nan))[k] == 0.0                            # not NaN
        assert fn(-1.0, 0.0, None)[k] == 0.0
        assert fn(0.5, 2.0, g0)[k] == 2.0 * g0[k]                                           # exactly beta * g
        others = np.delete(fn(1.0, 0.0, None), k)
        assert np.isfinite(others).all() and (others != 0.0).all()
    row, col = plan.entries()
    ref, mag = pair_reference(row, col, P, Q, in_pattern(plan))
    assert (np.abs(plan.values_grad_pairs_host(P, Q) - ref) <= 7 * U * mag).all()


def _plan_with_extra(tmp_path, S, i, j, v, name):
    import cholesky_amd as ca
    path = os.path.join(str(tmp_path), name + ".mtx")
    si.write_mtx(path, S.n, np.append(S.row, i), np.append(S.col, j), np.append(S.val, v))
    return ca.Plan(path, S.ord, S.clust)


def test_refused_plans(spd, tmp_path):
    import cholesky_amd as ca
    S = spd("lapl_25x25")
    n = S.n
    P = np.ones((n, 2))
    Za = np.ones(S.plan.arena_doubles)
    # a duplicated position: the first off-diagonal entry once more
    e = int(np.nonzero(S.row != S.col)[0][0])
    dup = _plan_with_extra(tmp_path, S, int(S.row[e]), int(S.col[e]), 0.25, "dup")
    assert dup.nz == S.plan.nz + 1 and dup.nnz_a == S.plan.nnz_a + 1 and dup.duplicate_entries == 1 and dup.dropped == 0
    # dropped entries: two dofs whose separators are not ancestor and descendant
    blocks = {(int(b[0]), int(b[1])) for b in S.plan.blocks}
    pos_sep = np.repeat(np.arange(1, S.plan.nsep + 1), S.plan.sep_sizes)[np.argsort(np.concatenate(
        [S.plan.sep_offsets[s] + np.arange(S.plan.sep_sizes[s]) for s in range(S.plan.nsep)]), kind="stable")]
    x, y = next((x, y) for x in range(n) for y in range(x) if (int(pos_sep[x]), int(pos_sep[y])) not in blocks and (int(pos_sep[y]), int(pos_sep[x])) not in blocks)
    i, j = int(S.perm[x]), int(S.perm[y])
    drop = _plan_with_extra(tmp_path, S, max(i, j), min(i, j), 0.125, "drop")
    assert drop.dropped == 1 and drop.duplicate_entries == 0
    for plan, word in ((dup, "repeat"), (drop, "dropped")):
        g = np.full(plan.nz, 3.0)
        with pytest.raises(ca.CholamdError, match=word) as ei:
            plan.values_grad_pairs_host(P, P, g=g)
        r, c = plan.entries()
        k = int(re.search(r"entry (\d+) at", str(ei.value)).group(1))                      # the message names the entry
        assert f"entry {k} at ({r[k]}, {c[k]})" in str(ei.value)
        assert (int(r[k]), int(c[k])) in {(int(S.row[e]), int(S.col[e])), (max(i, j), min(i, j))}
        with pytest.raises(ca.CholamdError, match=word):
            plan.values_grad_logdet_host(Za)
        out = np.full(plan.nz, 3.0)
        rc = plan.L.cholamd_plan_values_grad_pairs_host(plan.h, P.ctypes.data, n, P.ctypes.data, n, 1, 1.0, 0.0, out.ctypes.data, plan.nz)
        assert rc == -4 and (out == 3.0).all()                                              # nothing written


@pytest.mark.parametrize("name", si.NAMES)
def test_no_duplicates_on_the_suites_inputs(name, spd):
    assert spd(name).plan.duplicate_entries == 0


def test_no_duplicates_on_the_fixtures():
    import cholesky_amd as ca
    from conftest import CASES, case_paths
    for case in CASES:
        assert ca.Plan(*case_paths(case)[:3]).duplicate_entries == 0


def orig_reference(S, Zr):
    """(Zref in original order, the bound's r in original order): test_gpu_selinv's _orig_bound."""
    p = S.perm
    Zo = np.empty_like(Zr)
    Zo[np.ix_(p, p)] = Zr
    r = np.empty(S.n)
    r[p] = np.abs(Zr * S.sp[:, None] * S.sp[None, :]).sum(axis=1)
    return Zo, r


@pytest.mark.parametrize("name", INPUTS + ["lapl_400x400"])
def test_logdet_terms_over_the_models_z_arena(name, spd):
    S = spd(name)
    plan = S.plan
    Za = sr.model(plan, S.Lo)
    g = plan.values_grad_logdet_host(Za)
    row, col = plan.entries()
    assert in_pattern(plan).all() and np.isfinite(g).all()
    m = np.where(row == col, 1.0, 2.0)
    Zo, r = orig_reference(S, sr.zref(S.PAP, S.Ld))
    q = float(np.max(np.abs(g - m * Zo[row, col]) * S.s[row] * S.s[col] / (m * (S.k + 1) * U * r[row] * r[col])))
    print(f"logdet terms {name}: nz = {plan.nz}, max ratio = {q:.3g} (bound {sr.C_SEL})")
    assert q <= sr.C_SEL
    # exactly m_k times the arena's element, and alpha / beta as for the pair sums
    vm = plan.value_map()
    Zd = plan.arena_to_dense(np.nan_to_num(Za))
    pi = np.empty(S.n, dtype=np.int64)
    pi[S.perm] = np.arange(S.n)
    a, b = pi[row], pi[col]
    assert np.array_equal(g, m * Zd[np.maximum(a, b), np.minimum(a, b)]) and len(vm) == plan.nz
    g0 = np.random.default_rng(3).standard_normal(plan.nz)
    want = np.array([float(np.longdouble(0.5) * np.longdouble(t) + np.longdouble(2.0 * b0)) for t, b0 in zip(g, g0)])
    assert np.array_equal(plan.values_grad_logdet_host(Za, 0.5, 2.0, g=g0), want)


def test_the_reference_formulas_against_central_differences(spd):
    """The test's own reference, not the code under test: -sum_c lam_c^T E_k x_c and m_k Z_ij against central differences of numpy's dense solve
    and slogdet on lapl_25x25 with random values on the pattern."""
    S = spd("lapl_25x25")
    n = S.n
    row, col = S.plan.entries()
    v = np.array([S.A[i, j] for i, j in zip(row, col)])
    rng = np.random.default_rng(5)
    B, T = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))

    def dense(vals):
        A = np.zeros((n, n))
        A[row, col] = vals
        A[col, row] = vals
        return A

    assert np.array_equal(dense(v), S.A)
    A = dense(v)
    X, Lam, Z = np.linalg.solve(A, B), np.linalg.solve(A, T), np.linalg.inv(A)
    m = np.where(row == col, 1.0, 2.0)
    an_solve = -((Lam[row] * X[col]).sum(axis=1) + np.where(row != col, (Lam[col] * X[row]).sum(axis=1), 0.0))
    an_logdet = m * Z[row, col]
    fd_solve, fd_logdet = np.empty(len(v)), np.empty(len(v))
    for k in range(len(v)):
        h = 1e-5 * abs(v[k])
        f = []
        for sgn in (1.0, -1.0):
            w = v.copy()
            w[k] += sgn * h
            Aw = dense(w)
            f.append(((T * np.linalg.solve(Aw, B)).sum(), np.linalg.slogdet(Aw)[1]))
        fd_solve[k], fd_logdet[k] = (f[0][0] - f[1][0]) / (2 * h), (f[0][1] - f[1][1]) / (2 * h)
    e1 = float(np.abs(fd_solve - an_solve).max() / np.abs(an_solve).max())
    e2 = float(np.abs(fd_logdet - an_logdet).max() / np.abs(an_logdet).max())
    print(f"central differences: solve {e1:.3g}, logdet {e2:.3g} (gate 1e-6)")
    assert e1 <= 1e-6 and e2 <= 1e-6
    # ... and the library's pair sums are that formula
    g = S.plan.values_grad_pairs_host(Lam, X, alpha=-1.0)
    _, mag = pair_reference(row, col, Lam, X)
    assert (np.abs(g - an_solve) <= 2 * (2 * 3 + 1) * U * mag).all()                       # two fp64 sums of the same terms in different orders


def test_symbols_and_signatures():
    import cholesky_amd as ca
    from cholesky_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    L = ca.load()
    ctype = {"int64_t": C.c_int64, "int": C.c_int, "double": C.c_double}
    for name, params in SIGNATURES.items():
        mt = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert mt, f"{name} is not declared in the header"
        declared = [re.sub(r"\s+", " ", re.match(r"^(.*?)\w+$", a.strip()).group(1)).strip() for a in mt.group(1).split(",")]
        assert declared == params, (name, declared)
        fn = getattr(L, name)
        assert list(fn.argtypes) == [ctype.get(p, C.c_void_p) for p in params] and fn.restype is C.c_int
    assert re.search(r"\bint64_t\s+cholamd_plan_duplicate_entries\s*\(\s*const cholamd_plan \*\w+\)\s*;", text)
    for meth in ("values_grad_pairs", "values_grad_logdet"):
        assert callable(getattr(ca.Device, meth))
    assert callable(ca.factorize) and callable(ca.Factorization.solve) and callable(ca.Factorization.logdet) and callable(ca.Factorization.release)
    buf = np.zeros(4)
    p = buf.ctypes.data
    assert L.cholamd_values_grad_pairs(None, p, 4, p, 4, 1, 1.0, 0.0, p, 4, None) == -4 and b"NULL device" in L.cholamd_last_error()
    assert L.cholamd_values_grad_logdet(None, p, 1.0, 0.0, p, 4, None) == -4 and b"NULL device" in L.cholamd_last_error()
