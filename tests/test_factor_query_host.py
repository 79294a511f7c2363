"""Host side of the factor queries (cholamd_solve_half*, cholamd_factor_logdet*, cholamd_factor_diag*): the eight symbols with their declared
signatures, and the diagonal walk the kernels use (cholamd_plan_diag_list) checked against cholamd_plan_arena_to_dense -- no device needed."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import CASES, case_paths

SIGNATURES = {
    # name: C parameter types as the header declares them, in order
    "cholamd_solve_half": ["cholamd_device *", "const double *", "const double *", "double *", "int", "void *"],
    "cholamd_solve_half_f32": ["cholamd_device *", "const float *", "const double *", "double *", "int", "void *"],
    "cholamd_solve_half_nrhs": ["cholamd_device *", "const double *", "const double *", "int64_t", "double *", "int64_t", "int", "int", "void *"],
    "cholamd_solve_half_nrhs_f32": ["cholamd_device *", "const float *", "const double *", "int64_t", "double *", "int64_t", "int", "int", "void *"],
    "cholamd_factor_logdet": ["cholamd_device *", "const double *", "double *", "void *"],
    "cholamd_factor_logdet_f32": ["cholamd_device *", "const float *", "double *", "void *"],
    "cholamd_factor_diag": ["cholamd_device *", "const double *", "double *", "void *"],
    "cholamd_factor_diag_f32": ["cholamd_device *", "const float *", "double *", "void *"],
}


@pytest.fixture(scope="module")
def ca():
    import cholesky_amd
    return cholesky_amd


def _ctype(decl, name):
    """The ctypes type _lib.py must give a parameter declared as `decl` (logdet_out is the one pointer passed by reference from Python)."""
    if decl == "int":
        return C.c_int
    if decl == "int64_t":
        return C.c_int64
    if decl == "double *" and "logdet" in name:
        return C.POINTER(C.c_double)
    assert decl.endswith("*"), decl
    return C.c_void_p


def test_symbols_signatures_and_constants(ca):
    from cholesky_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    L = ca.load()
    for name, params in SIGNATURES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in the header"
        declared = [re.sub(r"\s+", " ", re.match(r"^(.*?)\w+$", a.strip()).group(1)).strip() for a in m.group(1).split(",")]
        assert declared == params, (name, declared)
        fn = getattr(L, name)
        assert fn.argtypes is not None and list(fn.argtypes) == [_ctype(p, name) for p in params], (name, fn.argtypes)
        assert fn.restype is C.c_int
    for macro, value in (("CHOLAMD_HALF_FORWARD", 0), ("CHOLAMD_HALF_BACKWARD", 1)):
        assert re.search(r"#define\s+" + macro + r"\s+" + str(value) + r"\b", text), macro
    assert (ca.HALF_FORWARD, ca.HALF_BACKWARD) == (0, 1)
    assert (ca.Device.HALF_FORWARD, ca.Device.HALF_BACKWARD) == (0, 1)
    for meth in ("solve_half", "solve_half_nrhs", "logdet", "factor_diag"):
        assert callable(getattr(ca.Device, meth))


def _plans(ca, tmp_path):
    for case in CASES:
        yield case, ca.Plan(*case_paths(case)[:3])
    for dims in ((7, 5, 3, 3, 4), (12, 12, 12, 4, 16), (20, 20, 1, 3, 16)):
        yield str(dims), ca.Problem(*dims).plan()


def test_diag_list_covers_every_position_once_and_addresses_the_diagonal(ca, tmp_path):
    for name, plan in _plans(ca, tmp_path):
        n = plan.n
        a_off, cols, lda, x_off, sep, prefix = plan.diag_list()
        assert len(a_off) == plan.nsep, name
        # every permuted position exactly once, in order
        assert prefix[0] == 0 and prefix[-1] == n and np.array_equal(np.diff(prefix), cols), name
        assert np.array_equal(x_off, prefix[:-1]), name
        assert sorted(sep) == list(range(1, plan.nsep + 1)), name
        assert np.array_equal(x_off, plan.sep_offsets[sep - 1]) and np.array_equal(cols, plan.sep_sizes[sep - 1]), name
        covered = np.zeros(n, dtype=np.int64)
        idx = np.empty(n, dtype=np.int64)               # arena index of L(p, p) by the walk's rule
        for i in range(len(a_off)):
            j = np.arange(cols[i], dtype=np.int64)
            covered[x_off[i] + j] += 1
            idx[x_off[i] + j] = a_off[i] + j * (int(lda[i]) + 1)
        assert (covered == 1).all(), name
        assert idx.min() >= 0 and idx.max() < plan.arena_doubles and len(np.unique(idx)) == n, name
        # a marker arena: position p's marker must land on (p, p) of the dense image, and nothing else is non-zero
        marker = np.zeros(plan.arena_doubles)
        marker[idx] = 1000.0 + np.arange(n)
        D = plan.arena_to_dense(marker)
        assert np.array_equal(np.diag(D), 1000.0 + np.arange(n)), name
        assert np.count_nonzero(D) == n, name
        # a matrix with a distinctive diagonal through the plan's own scatter: the walk reads A(perm[p], perm[p])
        host = plan.fill_host()
        assert np.array_equal(host[idx], np.diag(plan.arena_to_dense(host))), name


def test_distinctive_diagonal_through_fill_host(ca, tmp_path):
    """A with A_ii = 100 + i (original order): the walk over cholamd_plan_fill_host's arena returns 100 + perm[p] at position p."""
    import spd_inputs as si
    S = si.SPD(str(tmp_path), (7, 5, 3, 3, 4), 3, pattern="full", oracle=False, name="dq")
    n = S.n
    val = S.val.copy()
    val[:n] = 100.0 + np.arange(n)                     # the first n entries are the diagonal, in dof order
    si.write_mtx(S.mtx, n, S.row, S.col, val)
    plan = ca.Plan(S.mtx, S.ord, S.clust)
    a_off, cols, lda, x_off, _, _ = plan.diag_list()
    host = plan.fill_host()
    got = np.empty(n)
    for i in range(len(a_off)):
        j = np.arange(cols[i], dtype=np.int64)
        got[x_off[i] + j] = host[a_off[i] + j * (int(lda[i]) + 1)]
    assert np.array_equal(got, 100.0 + plan.perm)


def test_reference_quantities_agree_with_numpy_alone(tmp_path_factory):
    """The references the GPU tests use -- M = P^T Ld P and logdet_ref = 2 sum log diag(Ld) from the dense fp64 factor -- against numpy alone
    (M M^T = A in spd_inputs' reconstruction measure, numpy.linalg.slogdet of P A P^T) inside the bounds those tests apply, for every input
    they keep (all of spd_inputs.INPUTS, both precisions: the fp64 bound is the tighter one)."""
    import spd_inputs as si
    for name in si.NAMES:
        S = si.cached(tmp_path_factory, name)
        n, p = S.n, S.perm
        sign, ref = np.linalg.slogdet(S.PAP)
        ld = 2.0 * float(np.sum(np.log(np.diag(S.Ld))))
        tol = si.C_L * (S.k + 1) * si.U64 * S.kappa * n
        assert sign == 1.0 and abs(ld - ref) <= tol, (name, ld, ref, tol)
        M = np.zeros((n, n))
        M[np.ix_(p, p)] = S.Ld                                  # M = P^T Ld P: M[perm[i], perm[j]] = Ld[i, j]
        E = (M @ M.T - S.A) / S.s[:, None] / S.s[None, :]
        rec = float(np.linalg.norm(E) / np.linalg.norm(S.A / S.s[:, None] / S.s[None, :]))
        assert rec <= S.tol_reconstruction(), (name, rec)
        assert S.tol_forward(si.U64) < 1.0 and S.tol_factor(si.U64) < 1.0, name      # the fp64 bounds say something for every input
