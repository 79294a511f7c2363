"""Dof sets, references and gates of the sparse-solve tests (a helper module, not a conftest): tests/test_sparse_solve_host.py on the CPU and
tests/test_gpu_sparse_solve.py on the device share them, and the references of an (input, set) pair are computed once.

Inputs (tests/test_solve_det_host.py's Input class and its cache): tree_tiny (4 levels, 1-column separators: a path of width-1 spans), tree_skew (a
289-column, two-span separator at a leaf under 1-column ancestors), tree_top (433- and 289-column top: spans at col0 = 256 that survive without items),
tree_single (one separator, nothing to prune), g7_ragged, and the fixture lapl_3375x3375 (5 levels, 31 separators).

Sets, from Plan.perm / sep_offsets / sep_sizes / tree (heap index h: root 1, children 2 h and 2 h + 1):
  A  one dof of the first leaf                B  one dof of the root separator        C  one dof each in two sibling leaves
  D  one dof of a mid-level separator         E  in: first leaf, out: last leaf -- the paths meet at the root only, so up(out) \\ up(in) is not empty
  F  in: everything, out: A                   G  in: A, out: everything               H  both everything
A tree of one level has no siblings and no middle: C, D and E fall back to dofs of the one separator."""
import numpy as np

from spd_inputs import U64

INPUTS = ["tree_tiny", "tree_skew", "tree_top", "tree_single", "g7_ragged", "lapl_3375x3375"]
SETS = "ABCDEFGH"
NRHS = [1, 32, 33]
KMAX = 33


def sep_dofs(P, h):
    """The dofs (original ids) of the separator at heap index h, in permuted order."""
    lbl = int(P.tree[h - 1])
    o, m = int(P.sep_offsets[lbl - 1]), int(P.sep_sizes[lbl - 1])
    return np.asarray(P.perm[o:o + m], dtype=np.int64)


def mid(d):
    return d[len(d) // 2:len(d) // 2 + 1]


def dof_set(P, which):
    """(in_dofs, out_dofs) of set `which`."""
    L, ns = P.levels, P.nsep
    first_leaf, last_leaf = 1 << (L - 1), ns
    everything = np.arange(P.n, dtype=np.int64)
    a = mid(sep_dofs(P, first_leaf))
    if which == "A":
        return a, a
    if which == "B":
        b = mid(sep_dofs(P, 1))
        return b, b
    if which == "C":
        if L == 1:
            d = sep_dofs(P, 1)
            c = np.array([d[0], d[-1]])
        else:
            c = np.concatenate([mid(sep_dofs(P, first_leaf)), mid(sep_dofs(P, first_leaf + 1))])
        return c, c
    if which == "D":
        d = mid(sep_dofs(P, 1 << ((L - 1) // 2))) if L > 2 else sep_dofs(P, 1)[:1]
        return d, d
    if which == "E":
        return a, mid(sep_dofs(P, last_leaf)) if L > 1 else sep_dofs(P, 1)[-1:]
    if which == "F":
        return everything, a
    if which == "G":
        return a, everything
    assert which == "H"
    return everything, everything


def up(P, dofs):
    """Heap indices of the separators of `dofs` and their ancestors, from the plan's arrays alone."""
    iperm = np.empty(P.n, dtype=np.int64)
    iperm[np.asarray(P.perm, dtype=np.int64)] = np.arange(P.n)
    off = np.asarray(P.sep_offsets, dtype=np.int64)
    lbl = np.searchsorted(off, iperm[np.asarray(dofs, dtype=np.int64)], side="right")      # labels are numbered in the permuted order
    heap_of = {int(l): h + 1 for h, l in enumerate(P.tree)}
    out = set()
    for l in set(lbl.tolist()):
        h = heap_of[int(l)]
        while h >= 1:
            out.add(h)
            h >>= 1
    return out


def active_mask(P, heaps):
    """Boolean mask over permuted positions of the separators `heaps`."""
    m = np.zeros(P.n, dtype=bool)
    for h in heaps:
        lbl = int(P.tree[h - 1])
        o = int(P.sep_offsets[lbl - 1])
        m[o:o + int(P.sep_sizes[lbl - 1])] = True
    return m


_REF = {}


def dense_a(I):
    """A in original dof order (dense) and its COO triplets in long double, once per input."""
    key = (I.name, "dense A")
    if key not in _REF:
        if I.S is not None:
            A = np.asarray(I.S.A, dtype=np.float64)
        else:
            A = np.empty_like(I.PAP)
            A[np.ix_(I.perm, I.perm)] = I.PAP
        r, c = np.nonzero(A)
        _REF[key] = (A, r, c, A[r, c].astype(np.longdouble))
    return _REF[key]


def dense_solve(I, B):
    """A^-1 B from the dense factor of P A P^T with one correction from a long-double residual; original order."""
    import scipy.linalg as sl
    _, r, c, v = dense_a(I)
    p = np.asarray(I.perm, dtype=np.int64)

    def solve(R):
        X = np.empty_like(R)
        X[p] = sl.cho_solve((I.Ld, True), R[p])
        return X
    X = solve(B)
    R = B.astype(np.longdouble)
    np.subtract.at(R, r, v[:, None] * X.astype(np.longdouble)[c])
    return X + solve(R.astype(np.float64))


def case(I, which):
    """(in_dofs, out_dofs, Bs [n_in x KMAX], the scattered B [n x KMAX], its reference solution [n x KMAX]) of an input and a set, computed once.
    Bs: seeded normal columns scaled by the equilibration s = sqrt(diag A), as the block tests scale their right-hand sides."""
    key = (I.name, which)
    if key not in _REF:
        P = I.plan
        i, o = dof_set(P, which)
        Bs = I.s[i, None] * np.random.default_rng(500 + ord(which)).standard_normal((len(i), KMAX))
        B = np.zeros((P.n, KMAX))
        B[i] = Bs
        X = dense_solve(I, B)
        for a in (Bs, B, X):
            a.setflags(write=False)
        _REF[key] = (i, o, Bs, B, X)
    return _REF[key]


def tol_forward(I, u=U64):
    return I.S.tol_forward(u) if I.S is not None else I.tol_forward() * (u / U64)


def out_error(I, o, x, xref_full):
    """max_out |s (x - xref)| / max_all |s xref| of one column: x on the output dofs o against a reference on all dofs."""
    return float(np.abs(I.s[o] * (x - xref_full[o])).max() / np.abs(I.s * xref_full).max())


def column_gate(I, o, x, xref_full, tag, u=U64, factor=1.0):
    """The accuracy gate of one column on the output rows.  The trees: out_error <= factor tol_forward(u), tol_forward = C_FE (k + 1) u kappa
    (spd_inputs).  The Laplacian fixture in fp64: |x - xref|_max <= 1e-9 max(1, |xref|_max), the scale its other solve tests use; with an fp32 factor
    the fixture has no scale of its own and takes the trees' measure with its own k and kappa."""
    assert np.isfinite(x).all(), tag
    if I.S is None and u == U64:
        err, gate = float(np.abs(x - xref_full[o]).max()), factor * 1e-9 * max(1.0, float(np.abs(xref_full).max()))
    else:
        err, gate = out_error(I, o, x, xref_full), factor * tol_forward(I, u)
    print(f"{tag}: error {err:.3e} (gate {gate:.3e})")
    assert err <= gate, tag
