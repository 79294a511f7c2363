"""References for the forward products with the factor, y = M z and y = M^T z with M = P^T L P (a helper module, not a conftest).

The reference is tril(arena_to_dense(arena)) applied in numpy, in extended precision so that its own rounding does not take part of the gate.
The gate is the standard inner-product bound (Higham, Accuracy and Stability, section 3.1): a sum of k products computed in any order with unit
roundoff u = 2^-53 differs from the exact one by at most gamma_k |L| |z| <= (k + 2) u |L| |z| componentwise for the k of these inputs (k u << 1; the
two extra units cover gamma_k's denominator and the conversion of the reference back to fp64).  k = the most stored entries in a row of tril(L)
(FORWARD) or in a column (BACKWARD).  Nothing here is measured from the code under test."""
import numpy as np

U64 = 2.0 ** -53
FWD, BWD = 0, 1


def index_image(plan):
    """I (n x n, int64): I[i, j] = 1 + arena offset that holds position (i, j) of the permuted matrix, 0 where nothing is stored."""
    marks = np.arange(1, plan.arena_doubles + 1, dtype=np.float64)       # exact: the arenas of the test inputs are far below 2^53 elements
    return plan.arena_to_dense(marks).astype(np.int64)


def arena_from_lower(plan, L, fill=np.nan):
    """A host arena that holds tril(L) on the stored positions of the lower triangle and `fill` everywhere else: the upper triangles of the diagonal
    blocks, padding, whatever no block owns.  Entries of L without storage are dropped."""
    img = index_image(plan)
    arena = np.full(plan.arena_doubles, fill, dtype=np.float64)
    i, j = np.nonzero(np.tril(img))
    arena[img[i, j] - 1] = L[i, j]
    return arena


def stored_lower(plan, arena):
    """tril of the dense image of an arena (NaN above the diagonal is cut away), and the mask of its stored positions."""
    D = np.tril(plan.arena_to_dense(arena))
    return D, np.tril(index_image(plan)) != 0


def product(D, perm, z, which):
    """(y, |M| |z|) for M = P^T D P (FORWARD) or its transpose, in extended precision, rounded to fp64; original dof order."""
    Dl = D.astype(np.longdouble)
    T = Dl if which == FWD else Dl.T
    zp = np.asarray(z, dtype=np.float64)[perm].astype(np.longdouble)
    y, a = np.empty(len(perm)), np.empty(len(perm))
    y[perm] = (T @ zp).astype(np.float64)
    a[perm] = (np.abs(T) @ np.abs(zp)).astype(np.float64)
    return y, a


def longest(mask, which):
    """k of the gate: the most stored entries in a row (FORWARD) or a column (BACKWARD) of the lower triangle."""
    return int(mask.sum(axis=1 if which == FWD else 0).max())


def gate_ratio(y, yref, absprod, k, u=U64):
    """max_i |y - yref|_i / ((k + 2) u (|L| |z|)_i); a component whose bound is 0 must be exact."""
    bound = (k + 2) * u * absprod
    err = np.abs(y - yref)
    assert np.isfinite(y).all(), "the product is not finite"
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def product_sparse(Dsp, perm, z, which):
    """product() for tril(L) as a scipy CSR matrix (spd_inputs.arena_to_sparse): (y, |M| |z|, k), the sums in extended precision, k = the most
    non-zero terms of a component (exact zeros add no rounding, so this k is no larger than the stored count and the gate no wider)."""
    T = (Dsp if which == FWD else Dsp.T).tocsr()
    T.sort_indices()
    n = len(perm)
    zp = np.asarray(z, dtype=np.float64)[perm].astype(np.longdouble)
    prod = T.data.astype(np.longdouble) * zp[T.indices]
    cnt = np.diff(T.indptr)
    assert (cnt > 0).all(), "every row and column of a factor holds its diagonal entry"
    y, a = np.empty(n), np.empty(n)
    y[perm] = np.add.reduceat(prod, T.indptr[:-1]).astype(np.float64)
    a[perm] = np.add.reduceat(np.abs(prod), T.indptr[:-1]).astype(np.float64)
    return y, a, int(cnt.max())
