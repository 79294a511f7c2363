"""References and gates of the low-rank corrections (a helper module, not a conftest): builders of U, the numpy fp64 restatement of the formulas of
include/cholamd.h at "low-rank corrections", dense reference solves, and the gates.

Conventions (those of the header): M = P^T L P, Y = M^-1 U, G = Y^T Y, C = I + G (update), I - G (downdate), G (constraint), C = L_C L_C^T,
V = A^-1 U, W = V L_C^-T, A'^-1 = A^-1 - sigma W W^T with sigma = -1 for a downdate and +1 otherwise.

Well-conditioned U: U = P^T Ld Q K c with Ld the dense reference factor, Q (n x k) orthonormal (seeded), K = I + 0.25 N / ||N||_2 with N Gaussian.  Then
G = c^2 K^T K is dense and non-trivial in every tile, with eigenvalues in c^2 [0.5625, 1.5625]; c = 1 for update and constraint, 0.5 for downdate, so
kappa_2(C) <= 3 in every mode.  A diagonal G is never used: it would hide a transposed or misplaced off-diagonal tile.

Gates, all derived, u = 2^-53, none measured from the code under test:
 1. T = P^T Q against numpy: componentwise (n + 2) u (|P|^T |Q|) -- the inner-product bound, valid for any summation order.
 2. X = alpha X + beta V T: componentwise (k + 3) u (|alpha| |X| + |beta| |V| |T|).
 3. diag: (k + 2) u w_i.
 4. the corrected solve against the dense reference solve of A +- U U^T or of the KKT system (fp64 factor, two refinement steps, long-double residuals), in
    SPD.forward_error: 4 spd.tol_forward(u) kappa_2(C_ref) -- the plain solve, the two half solves behind W and the capacitance factor.  Conditions on the
    inputs (check_conditions): the numpy restatement is within a quarter of the gate, and ||S x_ref||_inf >= 0.25 ||S x0_ref||_inf (no cancellation hiding in
    the measure).  The constraint residual |U^T x - e| is gated componentwise by the same gate times (|U|^T |x| + |e|).
 5. logdet: |logdet_C - 2 sum log diag chol(C_ref)| <= 4 (k + 1) u kappa_2(C_ref) k."""
import numpy as np
import scipy.linalg as sl

from spd_inputs import U64

UPDATE, DOWNDATE, CONSTRAINT = 1, -1, 0
MODES = {"update": UPDATE, "downdate": DOWNDATE, "constraint": CONSTRAINT}
KS = [1, 15, 16, 17, 31, 32, 33, 70, 256]
NRHS = [1, 31, 32, 33]


def scale_of(mode):
    return 0.5 if mode == DOWNDATE else 1.0


def sigma_of(mode):
    return -1.0 if mode == DOWNDATE else 1.0


def build_u(spd, k, mode, seed=0, c=None):
    """U = P^T Ld Q K c (n x k, original dof order, Fortran order)."""
    rng = np.random.default_rng(7000 + 31 * seed + k)
    n = spd.n
    Q = np.linalg.qr(rng.standard_normal((n, k)))[0]
    N = rng.standard_normal((k, k))
    K = np.eye(k) + 0.25 * N / np.linalg.norm(N, 2)
    U = np.empty((n, k))
    U[spd.perm] = (spd.Ld @ (Q @ K)) * (scale_of(mode) if c is None else c)
    return np.asfortranarray(U)


def gaussian_u(spd, k, seed=0):
    """The generic case: seeded Gaussian columns scaled like the matrix (S N), no control of C."""
    rng = np.random.default_rng(9000 + seed)
    return np.asfortranarray(spd.s[:, None] * rng.standard_normal((spd.n, k)))


def half(spd, B, backward):
    """M^-1 B or M^-T B with the dense reference factor."""
    p = spd.perm
    out = np.empty_like(B)
    out[p] = sl.solve_triangular(spd.Ld, B[p], lower=True, trans="T" if backward else "N")
    return out


class Restated:
    """The numpy fp64 restatement of cholamd_lowrank_set and what follows from it."""

    def __init__(self, spd, U, mode):
        self.spd, self.U, self.mode, self.k = spd, U, mode, U.shape[1]
        k = self.k
        self.Y = half(spd, U, False)
        self.G = self.Y.T @ self.Y
        self.C = self.G if mode == CONSTRAINT else np.eye(k) + mode * self.G
        self.LC = np.linalg.cholesky(self.C)
        self.V = half(spd, self.Y, True)
        self.W = sl.solve_triangular(self.LC, self.V.T, lower=True).T
        self.kappa_c = float(np.linalg.cond(self.C, 2))
        self.logdet_c = 2.0 * float(np.log(np.diag(self.LC)).sum())
        self.w = (self.W * self.W).sum(axis=1)

    def plain(self, B):
        return half(self.spd, half(self.spd, B, False), True)

    def correction(self, B, E=None):
        """X - X0 = -sigma W t."""
        t = self.W.T @ B
        if self.mode == CONSTRAINT and E is not None:
            t = t - sl.solve_triangular(self.LC, E, lower=True)
        return -sigma_of(self.mode) * (self.W @ t)

    def solve(self, B, E=None):
        return self.plain(B) + self.correction(B, E)

    def project(self, x, e=None):
        r = self.U.T @ x - (0.0 if e is None else e)
        return x - self.W @ sl.solve_triangular(self.LC, r, lower=True)

    # -- gates ---------------------------------------------------------------------------------------
    def gate4(self):
        return 4.0 * self.spd.tol_forward(U64) * self.kappa_c

    def gate5(self):
        return 4.0 * (self.k + 1) * U64 * self.kappa_c * self.k


def a_times(spd, X):
    """A X in long double from the matrix file's entries (lower triangle and its mirror)."""
    ld = np.longdouble
    Xl, v, off = X.astype(ld), spd.val.astype(ld), spd.row != spd.col
    R = np.zeros(X.shape, dtype=ld)
    np.add.at(R, spd.row, v[:, None] * Xl[spd.col])
    np.add.at(R, spd.col[off], v[off, None] * Xl[spd.row[off]])
    return R


def reference_solve(spd, U, mode, B, E=None):
    """The dense reference: fp64 factor of A +- U U^T (Cholesky) or of the KKT matrix (LU), two refinement steps with the residual in long double (of the
    system as it is written: A from the matrix file's entries, U as given)."""
    n, k = U.shape
    ld = np.longdouble
    B = B.reshape(n, -1)
    Ul = U.astype(ld)
    if mode == CONSTRAINT:
        Kmat = np.zeros((n + k, n + k))
        Kmat[:n, :n], Kmat[:n, n:], Kmat[n:, :n] = spd.A, U, U.T
        rhs = np.vstack([B, np.zeros((k, B.shape[1])) if E is None else E.reshape(k, -1)])
        f = sl.lu_factor(Kmat)
        solve = lambda r: sl.lu_solve(f, r)  # noqa: E731
        resid = lambda z: rhs.astype(ld) - np.vstack([a_times(spd, z[:n]) + Ul @ z[n:].astype(ld), Ul.T @ z[:n].astype(ld)])  # noqa: E731
    else:
        rhs = B
        f = sl.cho_factor(spd.A + mode * (U @ U.T), lower=True)
        solve = lambda r: sl.cho_solve(f, r)  # noqa: E731
        resid = lambda z: rhs.astype(ld) - a_times(spd, z) - mode * (Ul @ (Ul.T @ z.astype(ld)))  # noqa: E731
    x = solve(rhs)
    for _ in range(2):
        x = x + solve(resid(x).astype(np.float64))
    return x[:n]


def ks_of(n):
    return sorted({min(k, n) for k in KS})


_PREP = {}


def prepare(S, name, mode, k, nrhs):
    """(U, restatement, B, E, Xref) of one case, once per session: everything the CPU can do before the device is asked, gate 4's conditions included."""
    key = (name, mode, k, nrhs)
    if key not in _PREP:
        U = build_u(S, k, mode)
        rs = Restated(S, U, mode)
        assert rs.kappa_c <= 3.0, rs.kappa_c
        rng = np.random.default_rng(500 + 7 * k + nrhs)
        B = np.asfortranarray(S.s[:, None] * rng.standard_normal((S.n, nrhs)))
        B[:, 0] = S.rhs
        E = None
        if mode == CONSTRAINT and (k % 2 == 1 or 4 * k > S.n):      # e != 0; with k near n and e = 0 the solution would vanish
            E = np.asfortranarray(0.5 * (U.T @ rs.plain(B)) * (1.0 + 0.1 * rng.standard_normal((k, nrhs))))
        Xref = reference_solve(S, U, mode, B, E)
        ratio = check_conditions(S, rs, B, Xref, E)
        _PREP[key] = (U, rs, B, E, Xref, ratio)
    return _PREP[key]


def forward_error(spd, X, Xref):
    """SPD.forward_error per column, the largest."""
    X, Xref = X.reshape(spd.n, -1), Xref.reshape(spd.n, -1)
    return max(spd.forward_error(X[:, j], Xref[:, j]) for j in range(X.shape[1]))


def check_conditions(spd, rs, B, Xref, E=None):
    """The conditions of gate 4 on an input, checked on the CPU: change the seed, not the gate, where one fails."""
    gate = rs.gate4()
    err = forward_error(spd, rs.solve(B, E), Xref)
    assert err <= 0.25 * gate, f"the numpy restatement misses a quarter of gate 4: {err:.3e} > {0.25 * gate:.3e}"
    X0 = rs.plain(B).reshape(spd.n, -1)
    Xr = Xref.reshape(spd.n, -1)
    for j in range(Xr.shape[1]):
        a, b = np.abs(spd.s * Xr[:, j]).max(), np.abs(spd.s * X0[:, j]).max()
        assert a >= 0.25 * b, f"column {j}: ||S x_ref|| = {a:.3e} < 0.25 ||S x0_ref|| = {0.25 * b:.3e}: cancellation hides in the measure"
    return err / gate


def constraint_ratio(rs, X, E=None):
    """max |U^T x - e| / (gate 4 (|U|^T |x| + |e|))."""
    X = X.reshape(rs.spd.n, -1)
    E = np.zeros((rs.k, X.shape[1])) if E is None else E.reshape(rs.k, -1)
    res = np.abs(rs.U.T @ X - E)
    den = rs.gate4() * (np.abs(rs.U).T @ np.abs(X) + np.abs(E))
    return float((res / den).max())


def gate1_ratio(T, P, Q):
    n = P.shape[0]
    ref = P.T @ Q
    bound = (n + 2) * U64 * (np.abs(P).T @ np.abs(Q))
    return _ratio(np.abs(T - ref), bound)


def gate2_ratio(X, alpha, X0, beta, V, T):
    k = V.shape[1]
    ref = alpha * X0 + beta * (V @ T) if alpha != 0.0 else beta * (V @ T)
    bound = (k + 3) * U64 * ((abs(alpha) * np.abs(X0) if alpha != 0.0 else 0.0) + abs(beta) * (np.abs(V) @ np.abs(T)))
    return _ratio(np.abs(X - ref), bound)


def gate3_ratio(w, W):
    k = W.shape[1]
    ref = (W * W).sum(axis=1)
    return _ratio(np.abs(w - ref), (k + 2) * U64 * ref)


def _ratio(err, bound):
    """max err / bound with 0 / 0 = 0."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert np.all(np.isfinite(err)), "a result is not finite"
    ok = bound > 0
    assert np.all(err[~ok] == 0.0), "an error where the bound is zero"
    return float((err[ok] / bound[ok]).max()) if ok.any() else 0.0
