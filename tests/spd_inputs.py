"""General symmetric positive-definite inputs for the factor and solve tests (a helper module, not a conftest).

Every reference fixture and every generated problem is a constant-coefficient grid Laplacian: a Stieltjes matrix, so every
off-diagonal entry of L is <= 0, every update product has one sign and the values of A are nearly all equal.  `build()` keeps a
base problem's nested-dissection ordering and cluster files and writes a new matrix file (`SPD`):

  base      a reference fixture, a generated grid (nx, ny, nz, levels, tile) or a synthetic elimination tree (a spec of tests/tree_inputs.py, which
            brings its own ordering, clusters and pattern: separator sizes no grid has)
  pattern   "own": the base's own pattern; "full": the 27-point stencil on the base's grid (9-point when nz == 1);
            "subset": each edge of that stencil kept with probability p (seeded)
  values    off-diagonal magnitudes log-uniform on [1e-2, 1e2], signs negative or mixed; diagonal sum_j |w_ij| + sigma
  scaling   D A D with D = 10^U(-s, s) (s = 0: none)

and returns the references an input needs: the dense P A P^T, its fp64 dense Cholesky factor, the CPU oracle's factor, a
right-hand side and a reference solution.

Measures (all invariant under a symmetric diagonal scaling of A):
  row_error(L, Lref, A)      max_ij |L - Lref|_ij / sqrt(A_ii)                  (|L_ij| <= sqrt(A_ii) for any SPD A)
  reconstruction(L, A)       ||S^-1 (L L^T - A) S^-1||_F / ||S^-1 A S^-1||_F with S = diag(A)^1/2
  backward_error(A, x, b)    max_i |b - A x|_i / (|A| |x| + |b|)_i
  forward_error(x, xref, A)  ||S (x - xref)||_inf / ||S xref||_inf

Tolerances (the tol_* methods of `SPD`): u is the unit roundoff of the arithmetic (2^-53 fp64, 2^-24 fp32), k the longest row of L
(the number of terms an entry of L L^T sums) and kappa the 2-norm condition number of the equilibrated matrix S^-1 A S^-1.
  * Cholesky is backward stable: L L^T = A + dA with |dA| <= gamma_(k+1) |L| |L^T| (Higham, Thm 10.3).  For the equilibrated
    matrix every entry of |L| |L^T| is <= 1 and the Frobenius norm of |L||L^T| is <= trace = n <= sqrt(n) ||A_eq||_F, so the
    reconstruction is <= gamma_(k+1) sqrt(n) ~ (k + 1) u sqrt(n): tol = C_REC (k + 1) u sqrt(n).
  * The forward error of L: a first-order perturbation of the factor is bounded by kappa times the relative backward error
    (Sun 1991, Higham Thm 10.8), so two factors of the same matrix (the one under test, the reference) differ per scaled entry by
    at most 2 kappa gamma_(k+1): tol = C_L (k + 1) u kappa.
  * A solve with the computed factor is backward stable with the same gamma (Higham Thm 10.4); componentwise: tol = C_BE (k + 1) u.
    The forward error is then bounded by kappa times that: tol = C_FE (k + 1) u kappa.
The constants C_* = 4 cover the two factors compared and the triangular solves' own rounding; the observed errors are orders of
magnitude below (error growth is like sqrt(k), not k)."""
import os

import numpy as np

from conftest import CASES, case_paths
from tree_inputs import NAMED as _TREE_NAMES, TREES as _TREES

U64 = 2.0 ** -53
U32 = 2.0 ** -24
C_REC = C_L = C_BE = C_FE = 4.0


def _read_coo(path):
    """Lower-triangle (row, col) 0-based and values of a coordinate Matrix-Market file (no comment lines after the banner)."""
    with open(path) as f:
        f.readline()
        n, _, nz = (int(v) for v in f.readline().split())
        d = np.loadtxt(f, ndmin=2)
    assert len(d) == nz
    i, j = d[:, 0].astype(np.int64) - 1, d[:, 1].astype(np.int64) - 1
    lo, hi = np.maximum(i, j), np.minimum(i, j)
    return n, lo, hi, d[:, 2]


def _stencil_edges(nx, ny, nz):
    """Lower-triangle edges (i > j) of the 27-point stencil (9-point when nz == 1) in the generator's numbering x + nx (y + ny z)."""
    x, y, z = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    x, y, z = x.ravel(), y.ravel(), z.ravel()
    j = x + nx * (y + ny * z)
    rows, cols = [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                xx, yy, zz = x + dx, y + dy, z + dz
                ok = (xx >= 0) & (xx < nx) & (yy >= 0) & (yy < ny) & (zz >= 0) & (zz < nz)
                i = xx + nx * (yy + ny * zz)
                ok &= i > j
                rows.append(i[ok])
                cols.append(j[ok])
    return np.concatenate(rows), np.concatenate(cols)


def write_mtx(path, n, row, col, val):
    """Lower triangle (row >= col, 0-based) sorted by (col, row), values with %.17g: the fp64 values round-trip exactly."""
    o = np.lexsort((row, col))
    with open(path, "w") as f:
        f.write("%%%%MatrixMarket matrix coordinate real symmetric\n%d %d %d\n" % (n, n, len(o)))
        f.writelines("%d %d %.17g\n" % (row[e] + 1, col[e] + 1, val[e]) for e in o)


class SPD:
    """One general SPD input: files, plan and references (see the module docstring)."""

    def __init__(self, tmp_path, base, seed, pattern="own", p=0.4, signs="mixed", sigma=1.0, scale=0.0, name="spd", oracle=True, dense=True):
        import cholesky_amd as ca
        rng = np.random.default_rng(seed)
        self.tree = None
        if isinstance(base, dict):       # a synthetic elimination tree (tests/tree_inputs.py): its own ordering, clusters and pattern
            import tree_inputs
            assert pattern == "own", "a tree spec names its own pattern"
            self.tree, self.ord, self.clust = tree_inputs.build(tmp_path, name, base)
            n, lo, hi = self.tree.n, self.tree.lo, self.tree.hi
        elif isinstance(base, str):
            m0, self.ord, self.clust, _ = case_paths(base)
            assert pattern == "own", "the fixtures are used with their own pattern"
            n, lo, hi, _ = _read_coo(m0)
        else:
            nx, ny, nz, levels, tile = base
            prob = ca.Problem(nx, ny, nz, levels, tile)
            m0, self.ord, self.clust, _ = prob.write(os.path.join(tmp_path, f"{name}_base"))
            n = prob.n
            if pattern == "own":
                _, lo, hi, _ = _read_coo(m0)
            else:
                lo, hi = _stencil_edges(nx, ny, nz)
        off = lo != hi
        r, c = lo[off], hi[off]
        if pattern == "subset":
            keep = rng.random(len(r)) < p
            r, c = r[keep], c[keep]
        w = 10.0 ** rng.uniform(-2.0, 2.0, len(r))
        if signs == "mixed":
            w *= np.where(rng.random(len(r)) < 0.5, -1.0, 1.0)
        else:
            w = -w
        diag = np.full(n, float(sigma))
        np.add.at(diag, r, np.abs(w))
        np.add.at(diag, c, np.abs(w))
        d = 10.0 ** rng.uniform(-scale, scale, n) if scale else np.ones(n)
        self.row = np.concatenate([np.arange(n), r])
        self.col = np.concatenate([np.arange(n), c])
        self.val = np.concatenate([diag * d * d, w * d[r] * d[c]])
        self.n, self.d, self.sigma = n, d, sigma
        self.mtx = os.path.join(tmp_path, f"{name}.mtx")
        write_mtx(self.mtx, n, self.row, self.col, self.val)
        self.plan = ca.Plan(self.mtx, self.ord, self.clust)
        assert self.plan.dropped == 0 and self.plan.n == n
        if self.tree is not None:        # the same arrays without the files: the same plan
            o = np.lexsort((self.row, self.col))
            self.plan_arrays = self.tree.plan_from_arrays(self.row[o], self.col[o], self.val[o])
            tree_inputs.assert_same_plan(self.plan, self.plan_arrays)
        self.perm = self.plan.perm
        # the original matrix, symmetric, and P A P^T built here (not by the library): PAP[i, j] = A[perm[i], perm[j]]; dense only with `dense`
        self.A_sparse = self.sparse_a()
        self.A = self.PAP = None
        if dense:
            self.A = self.A_sparse.toarray()
            self.PAP = self.A[np.ix_(self.perm, self.perm)]
        self.s = np.sqrt(self.A_sparse.diagonal())    # equilibration S = diag(A)^1/2, original order
        self.sp = self.s[self.perm]                   # ... permuted order
        self.rhs = self.s * rng.standard_normal(n)    # S^-1 b = O(1)
        self.Ld = np.linalg.cholesky(self.PAP) if dense else None
        self.Lo = None
        if oracle:
            from oracle import oracle as orc
            orc.use_own_kernels()
            O = orc.Oracle(self.mtx, self.ord, self.clust)
            O.factor()
            assert O.info == 0
            assert np.array_equal(O.perm, self.perm)
            self.Lo = np.tril(O.dense())
        if dense:
            self.x_ref = self.reference_solve(self.rhs)
            self.kappa = self.equilibrated_condition()
        self.k = self.longest_row()

    def sparse_a(self):
        """A (both triangles) as a scipy CSR matrix in the original order."""
        import scipy.sparse as sp
        n, off = self.n, self.row != self.col
        return sp.csr_matrix((np.concatenate([self.val, self.val[off]]), (np.concatenate([self.row, self.col[off]]),
                                                                          np.concatenate([self.col, self.row[off]]))), shape=(n, n))

    # -- references ---------------------------------------------------------------------------------
    def reference_solve(self, b):
        """fp64 dense Cholesky solve in P A P^T, two refinement steps with the residual in long double; original order."""
        import scipy.linalg as sl
        p = self.perm
        bp = b[p]
        Al = self.PAP.astype(np.longdouble)
        x = sl.cho_solve((self.Ld, True), bp)
        for _ in range(2):
            r = (bp.astype(np.longdouble) - Al @ x.astype(np.longdouble)).astype(np.float64)
            x = x + sl.cho_solve((self.Ld, True), r)
        out = np.empty_like(x)
        out[p] = x
        return out

    def equilibrated_condition(self, iters=60):
        """kappa_2(S^-1 A S^-1): lambda_max bounded above by Gershgorin, lambda_min from inverse iteration on the dense factor (an upper bound on
        lambda_min, converged to a few digits in 60 steps) -- a slight under-estimate at worst, covered by the constants C_*."""
        import scipy.linalg as sl
        sp = self.sp
        Ae = self.PAP / sp[:, None] / sp[None, :]
        lmax = np.abs(Ae).sum(axis=1).max()
        Le = self.Ld / sp[:, None]                      # the factor of the equilibrated matrix
        v = np.random.default_rng(0).standard_normal(self.n)
        mu = 0.0
        for _ in range(iters):
            v /= np.linalg.norm(v)
            y = sl.cho_solve((Le, True), v)
            mu = float(v @ y)
            v = y
        return lmax * mu

    def permuted_sparse(self):
        """P A P^T (both triangles) as a scipy CSR matrix."""
        p = self.perm
        return self.A_sparse[p][:, p].tocsr()

    def longest_row(self):
        """k: the most non-zeros in a row of L (of the dense reference's structure, else the oracle's)."""
        L = self.Ld if self.Ld is not None else self.Lo
        return None if L is None else int((L != 0).sum(axis=1).max())

    # -- measures -------------------------------------------------------------------------------------
    def row_error(self, L, Lref=None):
        Lref = self.Ld if Lref is None else Lref
        return float((np.abs(np.tril(L) - np.tril(Lref)) / self.sp[:, None]).max())

    def reconstruction(self, L):
        L = np.tril(L)
        E = (L @ L.T - self.PAP) / self.sp[:, None] / self.sp[None, :]
        return float(np.linalg.norm(E) / np.linalg.norm(self.PAP / self.sp[:, None] / self.sp[None, :]))

    def backward_error(self, x, b):
        Al = self.A.astype(np.longdouble)
        r = np.abs(b.astype(np.longdouble) - Al @ x.astype(np.longdouble))
        den = np.abs(Al) @ np.abs(x.astype(np.longdouble)) + np.abs(b.astype(np.longdouble))
        return float((r / den).max())

    def forward_error(self, x, xref=None):
        xref = self.x_ref if xref is None else xref
        return float(np.abs(self.s * (x - xref)).max() / np.abs(self.s * xref).max())

    def true_relres(self, x, b):
        """||b - A x||_2 / ||b||_2 (what cholamd_solve_refine reports), residual in long double."""
        r = b.astype(np.longdouble) - self.A.astype(np.longdouble) @ x.astype(np.longdouble)
        return float(np.sqrt((r * r).sum()) / np.linalg.norm(b))

    # -- tolerances -----------------------------------------------------------------------------------
    def tol_factor(self, u=U64):
        return C_L * (self.k + 1) * u * self.kappa

    def tol_reconstruction(self, u=U64):
        return C_REC * (self.k + 1) * u * np.sqrt(self.n)

    def tol_backward(self, u=U64):
        return C_BE * (self.k + 1) * u

    def tol_forward(self, u=U64):
        return C_FE * (self.k + 1) * u * self.kappa

    def refine_iterations(self, tol):
        """Iterations of fp32-factor refinement to bring ||b - A x||_2 / ||b||_2 to `tol`.  Every correction multiplies the scaled error S e
        (e = x - A^-1 b) by at most rho = C_FE (k + 1) u32 kappa (the forward error of one fp32 solve, < 1/2 where refinement is asked to
        converge), and the first solve starts at rho.  With A = S A_eq S: ||r|| = ||S A_eq S e|| <= s_max ||A_eq|| ||S e|| and
        ||b|| >= s_min lambda_min(A_eq) ||S x||, so the relative residual is at most (s_max / s_min) kappa sqrt(n) ||S e||_inf / ||S x||_inf:
        the error must fall to tol / ((s_max / s_min) kappa sqrt(n)).  Plus one for the last step's own rounding."""
        rho = self.tol_forward(U32)
        assert rho < 0.5, rho
        target = tol / (self.s.max() / self.s.min() * self.kappa * np.sqrt(self.n))
        return int(np.ceil(np.log(target) / np.log(rho))) + 1

    # -- layout ----------------------------------------------------------------------------------------
    def sep_of(self, pos):
        """(label, offset) of the separator holding permuted position pos."""
        off, size = self.plan.sep_offsets, self.plan.sep_sizes
        lbl = int(np.nonzero((off <= pos) & (pos < off + size))[0][0]) + 1
        return lbl, int(off[lbl - 1])

    def level_of(self, label):
        return self.plan.heap_of(label).bit_length() - 1


def arena_to_sparse(plan, arena):
    """tril of the matrix an arena holds (P A P^T or the factor L) as a scipy CSR matrix, read block by block through the plan's block table and
    tile maps (a 16-row tile without storage is zero) -- no dense n x n copy.  Equals tril(plan.arena_to_dense(arena)) with its zeros dropped."""
    import scipy.sparse as sp
    arena = np.asarray(arena, dtype=np.float64)
    rows, cols, vals = [], [], []
    for r, c, lo_x, lo_y, hi_x, hi_y, ld, off in plan.blocks:
        m, nc = int(hi_x - lo_x + 1), int(hi_y - lo_y + 1)
        tm = plan.block_tile_map(int(r), int(c))
        i = np.arange(m)
        t = tm[i // 16]
        keep = t >= 0
        i = i[keep]
        base = int(off) + t[keep].astype(np.int64) * 16 + i % 16
        for j0 in range(0, nc, 256):                  # column chunks: at most rows x 256 values at a time
            j = np.arange(j0, min(j0 + 256, nc))
            v = arena[base[:, None] + j[None, :] * int(ld)]
            mask = v != 0
            if r == c:
                mask &= i[:, None] >= j[None, :]
            ii, jj = np.nonzero(mask)
            rows.append(lo_x + i[ii])
            cols.append(lo_y + j[jj])
            vals.append(v[ii, jj])
    n = plan.n
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))


# the GPU suite's inputs: (id, base, options)
INPUTS = [
    ("lapl_9x9", "lapl_9x9", {}),
    ("lapl_25x25", "lapl_25x25", {}),
    ("lapl_400x400", "lapl_400x400", {}),
    ("lapl_3375x3375", "lapl_3375x3375", {}),
    ("lapl_3375_scaled", "lapl_3375x3375", {"scale": 3.0}),
    ("g12_full", (12, 12, 12, 4, 16), {"pattern": "full"}),
    ("g16_subset", (16, 16, 8, 3, 32), {"pattern": "subset", "p": 0.4}),
    ("g18_full", (18, 18, 18, 3, 48), {"pattern": "full"}),
    ("g20_2d", (20, 20, 1, 3, 16), {"pattern": "full"}),
    ("g7_ragged", (7, 5, 3, 3, 4), {"pattern": "full"}),
]
# synthetic trees (tests/tree_inputs.py), appended: the inputs above keep their seeds
INPUTS += [(nm, _TREES[nm], {}) for nm in _TREE_NAMES]
assert all(isinstance(b, (tuple, dict)) or b in CASES for _, b, _ in INPUTS)


NAMES = [nm for nm, _, _ in INPUTS]
_CACHE = {}


def make(tmp_path, name, seed=None):
    """The input `name` of INPUTS, seeded by its position in the list."""
    i = NAMES.index(name)
    _, base, opts = INPUTS[i]
    return SPD(tmp_path, base, 1000 + i if seed is None else seed, name=name, **opts)


def cached(tmp_path_factory, name, build=None):
    """make() once per test session (the references of the larger inputs take seconds).  `build(tmp_path)`: the maker of an input that is
    not in INPUTS (the single-purpose trees of tests/tree_inputs.py), cached under `name` in the same way."""
    if name not in _CACHE:
        tmp_path = tmp_path_factory.mktemp(name)
        _CACHE[name] = make(tmp_path, name) if build is None else build(tmp_path)
    return _CACHE[name]
