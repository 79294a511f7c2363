"""References, measure and CPU model of the selected inversion (a helper module for test_selinv_host.py and test_gpu_selinv.py, not a conftest).

Reference: Zref = (P A P^T)^-1, dense fp64: scipy Cholesky solves of the identity, two refinement steps with the residual I - A X in long double
(as SPD.reference_solve does; A is applied row-sparse, X in column chunks, so the long-double work is nnz(A) n and not n^3).

Measure and bound (the issue's): in the equilibrated matrix, S = diag(A)^1/2, Z_eq = S Z S (invariant under the scalings of spd_inputs).  A factor
with backward error dA gives, to first order, dZ = -Z dA Z, and with |dA_eq| <= gamma_(k+1) |L_eq||L_eq^T| <= gamma_(k+1) entrywise
|dZ_eq|_ij <= gamma_(k+1) r_i r_j, r_i = ||Z_eq[i, :]||_1.  Every checked entry is gated at C_SEL (k + 1) u r_i r_j, u = 2^-53, C_SEL = 2 x the
project's C_* = 4: the recursion's own products sum at most k terms of the same size a second time.  `ratio()` returns the largest observed
|dZ_eq|_ij / ((k + 1) u r_i r_j) over the mask; a NaN or inf anywhere on the mask makes it inf, so no entry of the mask can be left out.

Mask: the lower-triangle positions where the oracle's L is non-zero, plus the positions of tril(P A P^T).

CPU model: the recursion of chol_selinv.hip in numpy, column block by column block, taking the rows below every block and the "stored or not" answers
from the product's host view (Plan.selinv_front), reading 0.0 where the view says -1, on a Z arena that starts as NaN."""
import numpy as np

import spd_inputs as si
from conftest import case_paths

C_SEL = 2.0 * si.C_L


class Fixture:
    """One of the reference's four fixtures with its own values, carrying what SPD carries for the checks below."""

    def __init__(self, case):
        import cholesky_amd as ca
        from oracle import oracle as orc
        self.mtx, self.ord, self.clust, _ = case_paths(case)
        self.plan = ca.Plan(self.mtx, self.ord, self.clust)
        n, lo, hi, v = si._read_coo(self.mtx)
        A = np.zeros((n, n))
        A[lo, hi] = v
        A[hi, lo] = v
        self.n, self.A, self.perm = n, A, self.plan.perm
        self.PAP = A[np.ix_(self.perm, self.perm)]
        self.s = np.sqrt(np.diag(A))
        self.sp = self.s[self.perm]
        self.Ld = np.linalg.cholesky(self.PAP)
        orc.use_own_kernels()
        O = orc.Oracle(self.mtx, self.ord, self.clust)
        O.factor()
        assert O.info == 0
        self.Lo = np.tril(O.dense())
        self.k = int((self.Ld != 0).sum(axis=1).max())


def zref(PAP, Ld, chunk=256):
    """(P A P^T)^-1, dense fp64 (see the module docstring)."""
    import scipy.linalg as sl
    import scipy.sparse as sp
    n = PAP.shape[0]
    A = sp.csr_matrix(PAP)
    cnt = np.diff(A.indptr)
    mx = int(cnt.max())
    cols = np.zeros((n, mx), dtype=np.int64)
    vals = np.zeros((n, mx), dtype=np.longdouble)
    slot = np.arange(A.nnz) - np.repeat(A.indptr[:-1], cnt)
    rows = np.repeat(np.arange(n), cnt)
    cols[rows, slot] = A.indices
    vals[rows, slot] = A.data
    Z = np.empty((n, n))
    for c0 in range(0, n, chunk):
        c1 = min(n, c0 + chunk)
        E = np.zeros((n, c1 - c0))
        E[np.arange(c0, c1), np.arange(c1 - c0)] = 1.0
        X = sl.cho_solve((Ld, True), E)
        for _ in range(2):
            R = E.astype(np.longdouble)
            Xl = X.astype(np.longdouble)
            for t in range(mx):
                R -= vals[:, t, None] * Xl[cols[:, t], :]
            X = X + sl.cho_solve((Ld, True), R.astype(np.float64))
        Z[:, c0:c1] = X
    return 0.5 * (Z + Z.T)


def mask_of(S):
    """Lower-triangle positions to check: L_oracle != 0 plus tril(P A P^T) != 0; asserts that it contains every position of tril(P A P^T)."""
    a = np.tril(S.PAP) != 0
    m = (np.tril(S.Lo) != 0) | a
    assert not (a & ~m).any() and not np.triu(m, 1).any() and m.diagonal().all()
    return m


def ratio(S, Z, Zr, mask):
    """max over the mask of |Z - Zref|_eq,ij / ((k + 1) u r_i r_j); inf if any masked entry is not finite.  Also the share left out (0)."""
    sp = S.sp
    r = np.abs(Zr * sp[:, None] * sp[None, :]).sum(axis=1)
    i, j = np.nonzero(mask)
    z = Z[i, j]
    left_out = int(mask.sum()) - len(z)
    q = np.abs(z - Zr[i, j]) * sp[i] * sp[j] / ((S.k + 1) * si.U64 * r[i] * r[j])
    q = np.where(np.isfinite(z), q, np.inf)
    return float(q.max()), left_out


def offset_map(plan):
    """Dense n x n table: arena offset of position (i, j) by cholamd_plan_blocks + cholamd_plan_block_tile_map, -1 where nothing is stored."""
    n = plan.n
    OFF = np.full((n, n), -1, dtype=np.int64)
    for r, c, lo_x, lo_y, hi_x, hi_y, ld, off in plan.blocks:
        m, nc = int(hi_x - lo_x + 1), int(hi_y - lo_y + 1)
        tm = plan.block_tile_map(int(r), int(c))
        i = np.arange(m)
        t = tm[i // 16]
        keep = t >= 0
        i = i[keep]
        base = int(off) + t[keep].astype(np.int64) * 16 + i % 16
        j = np.arange(nc)
        OFF[(lo_x + i)[:, None], (lo_y + j)[None, :]] = base[:, None] + j[None, :] * int(ld)
    return OFF


def model(plan, L, OFF=None, on_front=None):
    """The recursion in numpy on a NaN-filled Z arena (see the module docstring); L: the permuted dense factor.  on_front(label, block, c0, nb, pos,
    off) is called for every front (the offset checks of the host test)."""
    import scipy.linalg as sl
    OFF = offset_map(plan) if OFF is None else OFF
    Za = np.full(plan.arena_doubles, np.nan)
    sizes = plan.sep_sizes
    for label in plan.tree:                              # heap order: root first, level by level
        label = int(label)
        if sizes[label - 1] == 0:
            continue
        for blk in reversed(range(plan.selinv_blocks(label))):
            c0, nb, pos, off = plan.selinv_front(label, blk)
            if on_front is not None:
                on_front(label, blk, c0, nb, pos, off)
            J = np.arange(c0, c0 + nb)
            X = sl.solve_triangular(L[np.ix_(J, J)], np.eye(nb), lower=True)
            ZJJ = X.T @ X
            if len(pos):
                Y = L[np.ix_(pos, J)] @ X
                Zbb = np.where(off >= 0, Za[np.maximum(off, 0)], 0.0)
                ZbJ = -Zbb @ Y
                dst = OFF[pos[:, None], J[None, :]]
                assert (dst >= 0).all()
                Za[dst] = ZbJ
                ZJJ -= Y.T @ ZbJ
            ii, jj = np.tril_indices(nb)
            dst = OFF[J[ii], J[jj]]
            assert (dst >= 0).all()
            Za[dst] = ZJJ[ii, jj]
    return Za
