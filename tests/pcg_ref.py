"""Reference for the preconditioned conjugate gradients of cholamd_solve_pcg (a helper module, not a conftest).

`pcg()` restates the library's loop in numpy: M^-1 is a dense cho_solve with a SUPPLIED lower factor (the fp64 factor of the factored values A, or its
float32 rounding's), the recurrences are the textbook ones, a column claims convergence when the recurrence's ||r||^2 <= tol^2 ||b||^2, the true
residual (long double) then decides, and where it does not agree it replaces r and the loop runs on with p = z.  The status codes are the library's.

Names: A are the values the factor was made from, A' (`Ap`) the values in force.  `Case` holds one pair on an input of spd_inputs: the value array of A'
in the plan's entry order, the dense A and A', and the gates of the tests.  The perturbations:

  scaled()     A' = 3 A                               one distinct eigenvalue of M^-1 A': one step in exact arithmetic
  rank(m)      A' = A + m diagonal increments         m + 1 distinct eigenvalues: m + 1 steps in exact arithmetic
  drift()      A' = A + 0.1 diag(a_ii xi_i)           xi uniform in [0, 1]: the classical bound with kp = kappa(M^-1 A')
  indefinite() A' = A with one diagonal entry negated and scaled so that e_i^T A' e_i < 0
"""
import numpy as np

import spd_inputs as si

TOL = 1e-12
MAX_ITER = 50
U64 = 2.0 ** -53
CONVERGED, MAXITER, BREAKDOWN, NAN = 0, 1, 2, 3

# the GPU inputs: fixtures and inputs of spd_inputs by name, two generated 2-D grids of n = 256 (one full workgroup of rows) and n = 255
GRIDS = {"g16x16": (16, 16, 1, 3, 16), "g17x15": (17, 15, 1, 3, 16)}
GPU_INPUTS = ["lapl_9x9", "lapl_25x25", "g16x16", "g17x15", "lapl_400x400", "g7_ragged", "tree_over"]
BIG = "lapl_3375x3375"


def spd(tmp_path_factory, name):
    """The input `name`, made once per session as spd_inputs makes its own."""
    if name in GRIDS:
        return si.cached(tmp_path_factory, name, build=lambda tmp: si.SPD(str(tmp), GRIDS[name], 4000 + sorted(GRIDS).index(name), pattern="full", name=name, oracle=False))
    return si.cached(tmp_path_factory, name)


def order(S):
    return np.lexsort((S.row, S.col))


def values(S):
    """The value array of S: its values in the order of its matrix file (= plan.entries())."""
    return np.ascontiguousarray(S.val[order(S)])


def dense_of(plan, vals):
    """The symmetric dense matrix of a value array on the plan's entries (original dof order)."""
    r, c = plan.entries()
    A = np.zeros((plan.n, plan.n))
    np.add.at(A, (r, c), vals)
    off = r != c
    np.add.at(A, (c[off], r[off]), vals[off])
    return A


def lower_factor(A, dtype=np.float64):
    """The dense lower Cholesky factor of A rounded to dtype first (float32: the stand-in of the fp32 arena), returned in fp64."""
    return np.linalg.cholesky(A.astype(dtype)).astype(np.float64)


def long_double(A):
    """A (dense fp64) as a sparse long-double matrix: the residuals of the reference (numpy's dense long-double product is slow)."""
    import scipy.sparse as sp
    return sp.csr_matrix(A).astype(np.longdouble)


def relres_ld(A, x, b):
    """||b - A x||_2 / ||b||_2 with the residual in long double (A: dense fp64, or long_double(A))."""
    Al = long_double(A) if isinstance(A, np.ndarray) else A
    r = b.astype(np.longdouble) - Al @ x.astype(np.longdouble)
    return float(np.sqrt((r * r).sum()) / np.sqrt((b.astype(np.longdouble) ** 2).sum()))


def pcg(A, L, b, tol=TOL, max_iter=MAX_ITER, x0=None, Al=None):
    """(x, iters, relres, status) of the loop of cholamd_solve_pcg on dense A with M = L L^T.  Al: long_double(A), if the caller has it."""
    import scipy.linalg as sl
    n = len(b)
    minv = lambda v: sl.cho_solve((L, True), v)  # noqa: E731
    Al = long_double(A) if Al is None else Al
    true_r = lambda x: (b.astype(np.longdouble) - Al @ x.astype(np.longdouble)).astype(np.float64)  # noqa: E731
    bb = float(b @ b)
    if bb == 0.0:
        return np.zeros(n), 0, 0.0, CONVERGED
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
    r = b.copy() if x0 is None else true_r(x)
    rel = float(np.sqrt((r @ r) / bb))
    if not np.isfinite(rel):
        return x, 0, rel, NAN
    if rel <= tol:
        return x, 0, rel, CONVERGED
    iters, status, fresh, rho, p = 0, MAXITER, True, 0.0, None
    while iters < max_iter:
        z = minv(r)
        rho_new = float(r @ z)
        if not np.isfinite(rho_new):
            status = NAN
            break
        if not rho_new > 0.0:
            status = BREAKDOWN
            break
        p = z if fresh else z + (rho_new / rho) * p
        fresh, rho = False, rho_new
        q = A @ p
        iters += 1
        sigma = float(p @ q)
        if not np.isfinite(sigma):
            status = NAN
            break
        if not sigma > 0.0:
            status = BREAKDOWN
            break
        alpha = rho / sigma
        x = x + alpha * p
        r = r - alpha * q
        rr = float(r @ r)
        if not np.isfinite(rr):
            status = NAN
            break
        if rr <= tol * tol * bb:  # the claim; the true residual decides
            t = true_r(x)
            if np.sqrt((t @ t) / bb) <= tol:
                status = CONVERGED
                break
            r, fresh = t, True
    return x, iters, relres_ld(Al, x, b), status


class Case:
    """One (A, A') pair on an input S: vals = the value array of A', A / Ap dense in original dof order."""

    def __init__(self, S, vals, kind):
        self.S, self.kind = S, kind
        self.vals0, self.vals = values(S), np.ascontiguousarray(vals)
        self.A, self.Ap = dense_of(S.plan, self.vals0), dense_of(S.plan, self.vals)
        self.nnz_row = int((self.Ap != 0).sum(axis=1).max())
        self._L, self._Lp, self._Apl, self._kappa2, self._kp = {}, None, None, None, None

    def L(self, dtype=np.float64):
        key = np.dtype(dtype).name
        if key not in self._L:
            self._L[key] = lower_factor(self.A, dtype)
        return self._L[key]

    def pcg(self, b, f32=False, **kw):
        """the reference loop on A' with the factor of A (f32: of A rounded to float32)"""
        return pcg(self.Ap, self.L(np.float32 if f32 else np.float64), b, Al=self.Apl(), **kw)

    def rhs(self, k=1, seed=0):
        """n x k right-hand sides scaled like spd_inputs' (S^-1 b = O(1))."""
        rng = np.random.default_rng(seed)
        return self.S.s[:, None] * rng.standard_normal((self.S.n, k))

    def x_star(self, b):
        """A'^-1 b: dense fp64 Cholesky of A' with two refinement steps in long double (spd_inputs.reference_solve on A')."""
        import scipy.linalg as sl
        if self._Lp is None:
            self._Lp = np.linalg.cholesky(self.Ap)
        Lp, Al, bl = self._Lp, self.Apl(), b.astype(np.longdouble)
        x = sl.cho_solve((Lp, True), b)
        for _ in range(2):
            x = x + sl.cho_solve((Lp, True), (bl - Al @ x.astype(np.longdouble)).astype(np.float64))
        return x

    def Apl(self):
        if self._Apl is None:
            self._Apl = long_double(self.Ap)
        return self._Apl

    def kappa2(self):
        if self._kappa2 is None:
            w = np.linalg.eigvalsh(self.Ap)
            self._kappa2 = float(w[-1] / w[0])
        return self._kappa2

    def kp(self):
        """lambda_max / lambda_min of the pencil (A', A): the eigenvalues of L^-1 A' L^-T."""
        import scipy.linalg as sl
        if self._kp is None:
            L = self.L()
            W = sl.solve_triangular(L, self.Ap, lower=True)
            W = sl.solve_triangular(L, W.T, lower=True)
            w = np.linalg.eigvalsh(0.5 * (W + W.T))
            self._kp = float(w[-1] / w[0])
        return self._kp

    def drift_bound(self, tol=TOL):
        """Steps after which the classical bound ||e_k||_A' <= 2 c^k ||e_0||_A' has brought the relative residual under tol:
        ||r_k|| / ||b|| <= sqrt(kappa_2(A')) ||e_k||_A' / ||e_0||_A' (x_0 = 0), so k = ceil(log(tol / (2 sqrt(kappa_2))) / log c)."""
        kp = self.kp()
        c = (np.sqrt(kp) - 1.0) / (np.sqrt(kp) + 1.0)
        return int(np.ceil(np.log(tol / (2.0 * np.sqrt(self.kappa2()))) / np.log(c)))

    # -- the gates of converged columns --------------------------------------------------
    def relres_slack(self, x, b):
        """How far a device ||b - A' x|| / ||b|| computed in fp64 with fma over at most nnz_row terms (plus the norm's own sum) may lie from the
        long-double one: (nnz_row + 2) u || |A'| |x| || / ||b||."""
        return (self.nnz_row + 2) * U64 * float(np.linalg.norm(np.abs(self.Ap) @ np.abs(x))) / float(np.linalg.norm(b))

    def check_converged(self, x, b, relres_out, tol=TOL, kappa=None, x_star=None):
        assert relres_out <= tol, (self.kind, relres_out)
        mine = relres_ld(self.Apl(), x, b)
        assert abs(mine - relres_out) <= self.relres_slack(x, b), (self.kind, mine, relres_out)
        kappa = self.kappa2() if kappa is None else kappa
        xs = self.x_star(b) if x_star is None else x_star
        err = float(np.linalg.norm(x - xs) / np.linalg.norm(xs))
        assert err <= kappa * mine, (self.kind, err, kappa, mine)


def _diag_index(plan):
    """value-array index of the diagonal entry of every row"""
    r, c = plan.entries()
    k = np.nonzero(r == c)[0]
    out = np.empty(plan.n, dtype=np.int64)
    out[r[k]] = k
    return out


def scaled(S, factor=3.0):
    return Case(S, factor * values(S), f"{factor:g} A")


def rank(S, m, seed=21):
    """m diagonal increments of 0.5 to 4 times a_ii on distinct rows.  In floating point the m + 1 steps of exact arithmetic hold only while the Lanczos
    vectors stay orthogonal; with m = 8 outlying eigenvalues the reference loop needs m + 2 or m + 3 steps on the smallest inputs, whichever rows are
    drawn.  The seed is one at which it needs at most m + 2 everywhere, which tests/test_pcg_host.py asserts."""
    rng = np.random.default_rng(seed + m)
    v, dg = values(S), _diag_index(S.plan)
    rows = rng.choice(S.n, size=m, replace=False)
    v[dg[rows]] *= 1.0 + rng.uniform(0.5, 4.0, m)
    return Case(S, v, f"rank {m}")


NRHS = [1, 5, 31, 32, 33]


def nrhs_of(name):
    """the column count of the input `name` in the scaled, drift and apply tests: round NRHS in the order of the inputs"""
    return NRHS[(GPU_INPUTS + [BIG]).index(name) % len(NRHS)]


def drift_nrhs(name):
    """the column count of the drift test: two on the big input, whose dense reference is the slow part"""
    return 2 if name == BIG else nrhs_of(name)


def rank_inputs(S, name, m):
    """(case, B) of the rank-m test on the input `name`: the column counts go round NRHS, so that the two smallest inputs -- where m = 8 outliers leave the
    cap m + 2 no slack (see rank()) -- meet it with 1 and 5 columns."""
    case = rank(S, m)
    return case, case.rhs(NRHS[(GPU_INPUTS.index(name) + {1: 1, 3: 2, 8: 0}[m]) % len(NRHS)])


def drift(S, seed=11, size=0.1):
    rng = np.random.default_rng(seed)
    v, dg = values(S), _diag_index(S.plan)
    v[dg] *= 1.0 + size * rng.uniform(0.0, 1.0, S.n)
    return Case(S, v, "drift")


def indefinite(S, row=None):
    """(case, row): the diagonal entry of `row` negated and doubled: e_i^T A' e_i = -2 a_ii < 0"""
    row = S.n // 2 if row is None else row
    v, dg = values(S), _diag_index(S.plan)
    v[dg[row]] *= -2.0
    return Case(S, v, "indefinite"), row
