"""Sparse solves on the device (cholamd_sparse_*, cholesky_amd.SparseSolve): right-hand sides on a few dofs, solutions on a few dofs, through the block
kernels of the deterministic solve on step lists pruned to the separators of those dofs and their ancestors.  Every test creates a SparseSolve handle, so
none passes on a library without the feature.

Inputs, dof sets and references: tests/sparse_sets.py (the smallest trees on which each pruning rule can go wrong, g7_ragged and the fixture
lapl_3375x3375; sets A .. H; 1, 32 and 33 columns, the last at ldb = n_in + 3 and ldx = n_out + 3).

Gates -- none is measured from the code under test:
  * accuracy, per column, fp64 and fp32 arenas with u = 2^-53 / 2^-24: max_out |s (x - xref)| / max_all |s xref| <= tol_forward(u) against the dense solve of
    the scattered b with one long-double correction (the Laplacian in fp64: 1e-9 max(1, |xref|_max)); G and H also backward_error <= tol_backward(u);
    against Device.solve_nrhs / solve_half_nrhs (both deterministic options on) of the scattered dense B at the output rows within TWICE the gate, since
    each of the two is within the gate of the truth.  The FORWARD half lives in the equilibrated system (L^-1 P b = (S^-1 L)^-1 S^-1 P b): its measure
    carries no scale.  FORWARD outputs outside up(in) are +0.0 exactly.
  * bits (torch.equal): contract (c) for H against solve_nrhs / solve_half_nrhs; (a) two calls, two handles, a device object created under
    CHOLAMD_POISON=1, a call right after a dense block solve of random data on the same device object; (b) a column alone, and beside NaN columns.
  * nothing inactive is read: the arena with NaN in every element that the handle's lists do not address gives the bits of the clean arena.
  * caller memory (tests/guarded.py): guards, padding rows, columns past nrhs untouched; Bs unchanged; in place where n_in == n_out."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import sparse_sets as ss  # noqa: E402
from guarded import Guarded  # noqa: E402
from spd_inputs import U32, U64  # noqa: E402
from test_solve_det_host import inputs  # noqa: E402,F401  (the shared input cache)

FWD, BWD, BOTH = 0, 1, -1
PRECISIONS = [False, True]
PIDS = ["fp64", "fp32"]
COUNTS = [(1, 0), (32, 0), (33, 3)]   # (columns, ld - rows)


@pytest.fixture(autouse=True)
def environment(monkeypatch):
    for v in ("CHOLAMD_POISON", "CHOLAMD_COMPACT", "CHOLAMD_SOLVE_NO_BAND", "CHOLAMD_SOLVE_NO_INV256", "CHOLAMD_SOLVE_REFERENCE_SHAPE", "CHOLAMD_SOLVE_DETERMINISTIC",
              "CHOLAMD_SOLVE_DETERMINISTIC_BLOCK"):
        monkeypatch.delenv(v, raising=False)


_FACT = {}


def switch_on(dev):
    dev.set_option("solve_reference_shape", 0)
    dev.set_option("solve_deterministic", 1)
    dev.set_option("solve_deterministic_block", 1)


def factored(I, f32):
    """(device object with both deterministic options on -- the comparison solves' -- and the factored arena), once per input and precision."""
    import cholesky_amd as ca
    key = (I.name, f32)
    if key not in _FACT:
        dev = ca.Device(I.plan, 0)
        a = dev.new_arena_f32() if f32 else dev.new_arena()
        (dev.fill_f32 if f32 else dev.fill)(a)
        (dev.factor_f32 if f32 else dev.factor)(a)
        dev.sync()
        assert dev.info() == (0, 0)
        switch_on(dev)
        _FACT[key] = (dev, a)
    return _FACT[key]


def block(M, pad=0, fill=None):
    """M (numpy, m x k) as a column-major device block at leading dimension m + pad; fill: every element starts as this value instead (an output)."""
    import torch
    m, k = M.shape
    buf = torch.full((k, m + pad), float("nan") if fill is None else fill, dtype=torch.float64, device="cuda")
    t = buf[:, :m].T
    if fill is None:
        t.copy_(torch.from_numpy(np.array(M, dtype=np.float64, order="C")).cuda())
    return t


def run(h, a, Bs, n_out, which=BOTH, pad=0):
    """The handle's solve of the columns of Bs (numpy) into a fresh block; the device tensor."""
    X = block(np.zeros((n_out, Bs.shape[1])), pad, fill=float("nan"))
    h.solve_nrhs(a, block(Bs, pad), X, which)
    h.dev.sync()
    return X


def dense(dev, a, B, which=BOTH):
    X = block(np.zeros(B.shape), 0, fill=float("nan"))
    if which == BOTH:
        dev.solve_nrhs(a, block(B), X)
    else:
        dev.solve_half_nrhs(a, block(B), X, which)
    dev.sync()
    return X


# ------------------------------------------------------------------------------------------------
# 1.  accuracy
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("which", list(ss.SETS))
@pytest.mark.parametrize("name", ss.INPUTS)
def test_solution_on_the_output_dofs(name, which, f32, inputs):
    import cholesky_amd as ca
    I = inputs(name)
    P = I.plan
    dev, a = factored(I, f32)
    u = U32 if f32 else U64
    i, o, Bs, B, Xref = ss.case(I, which)
    h = ca.SparseSolve(dev, i, o)
    assert h.counts() == P.sparse_counts(i, o)
    for k, pad in COUNTS:
        X = run(h, a, Bs[:, :k], len(o), BOTH, pad).cpu().numpy()
        assert X.shape == (len(o), k)
        for j in range(k):
            ss.column_gate(I, o, X[:, j], Xref[:, j], f"{name} set {which} {'fp32' if f32 else 'fp64'} nrhs={k} column {j}", u)
            if which in "GH" and I.S is not None:
                be = I.S.backward_error(X[:, j], B[:, j])
                assert be <= I.S.tol_backward(u), (name, which, j, be)
    # against the dense block solve of the scattered B at the output rows (X: the 33-column call)
    Xc = dense(dev, a, B).cpu().numpy()
    for j in range(ss.KMAX):
        ss.column_gate(I, o, X[:, j], Xc[:, j], f"{name} set {which} column {j} against Device.solve_nrhs", u, factor=2.0)
    # the halves
    tol = 2.0 * ss.tol_forward(I, u)
    p = np.asarray(I.perm, dtype=np.int64)
    iperm = np.empty(P.n, dtype=np.int64)
    iperm[p] = np.arange(P.n)
    act_fw, act_bw = ss.active_mask(P, ss.up(P, i)), ss.active_mask(P, ss.up(P, o))
    Y = run(h, a, Bs, len(o), FWD).cpu().numpy()
    Yc = dense(dev, a, B, FWD).cpu().numpy()
    outside = ~act_fw[iperm[o]]
    assert np.isfinite(Y).all() and (Y[outside] == 0.0).all() and not np.signbit(Y[outside]).any(), (name, which, "FORWARD outputs outside up(in) are not +0.0")
    ef = np.abs(Y - Yc[o]).max() / np.abs(Yc).max()
    Z = run(h, a, Bs, len(o), BWD).cpu().numpy()
    Zc = dense(dev, a, np.where(act_bw[iperm][:, None], B, 0.0), BWD).cpu().numpy()      # an input outside up(out) cannot reach a wanted output
    eb = np.abs(I.s[o, None] * (Z - Zc[o])).max() / max(np.abs(I.s[:, None] * Zc).max(), np.finfo(float).tiny)
    print(f"{name} set {which}: halves against Device.solve_half_nrhs: forward {ef:.3e}, backward {eb:.3e} (gate {tol:.3e})")
    assert np.isfinite(Z).all() and ef <= tol and eb <= tol
    h.close()


# ------------------------------------------------------------------------------------------------
# 2.  (c) everything active: the bits of the deterministic block solve
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("name", ss.INPUTS)
def test_everything_active_has_the_block_solves_bits(name, f32, inputs):
    import cholesky_amd as ca
    import torch
    I = inputs(name)
    dev, a = factored(I, f32)
    i, o, Bs, B, _ = ss.case(I, "H")
    h = ca.SparseSolve(dev, i, o)
    for which in (BOTH, FWD, BWD):
        for k, pad in COUNTS:
            X = run(h, a, Bs[:, :k], len(o), which, pad)
            assert torch.isfinite(X).all() and torch.equal(X, dense(dev, a, B[:, :k], which)), (name, which, k)
    h.close()


# ------------------------------------------------------------------------------------------------
# 3.  (a) the same bits every time
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("name", ss.INPUTS)
def test_bits_repeat(name, f32, inputs, monkeypatch):
    import cholesky_amd as ca
    import torch
    I = inputs(name)
    dev, a = factored(I, f32)
    monkeypatch.setenv("CHOLAMD_POISON", "1")              # read at every allocation of the library: this object's buffers start as NaN
    devp = ca.Device(I.plan, 0)
    noise = np.random.default_rng(9).standard_normal((I.plan.n, 33))
    for which in "AEH":
        i, o, Bs, _, _ = ss.case(I, which)
        monkeypatch.delenv("CHOLAMD_POISON", raising=False)
        h, h2 = ca.SparseSolve(dev, i, o), ca.SparseSolve(dev, i, o)
        monkeypatch.setenv("CHOLAMD_POISON", "1")
        hp = ca.SparseSolve(devp, i, o)
        for w in (BOTH, FWD, BWD):
            first = run(h, a, Bs, len(o), w, 3)
            assert torch.isfinite(first).all()
            assert torch.equal(run(h, a, Bs, len(o), w, 3), first), (which, w, "two calls return other bits")
            assert torch.equal(run(h2, a, Bs, len(o), w), first), (which, w, "a second handle returns other bits")
            assert torch.equal(run(hp, a, Bs, len(o), w), first), (which, w, "poisoned buffers change the bits")
            dense(dev, a, noise)                           # leaves stale non-zeros in every row of the device object's block
            assert torch.equal(run(h, a, Bs, len(o), w), first), (which, w, "what an earlier call left in the block changes the bits")
        for x in (h, h2, hp):
            x.close()
    monkeypatch.delenv("CHOLAMD_POISON")


# ------------------------------------------------------------------------------------------------
# 4.  (b) column independence
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["A", "C", "E", "F"])
@pytest.mark.parametrize("name", ["tree_tiny", "tree_skew", "lapl_3375x3375"])
def test_columns_are_independent(name, which, inputs):
    import cholesky_amd as ca
    import torch
    I = inputs(name)
    dev, a = factored(I, False)
    i, o, Bs, _, _ = ss.case(I, which)
    h = ca.SparseSolve(dev, i, o)
    Bn = Bs.copy()
    Bn[:, 7] = np.nan
    Bn[0, 32] = np.nan
    keep = [j for j in range(ss.KMAX) if j not in (7, 32)]
    for w in (BOTH, FWD, BWD):
        X = run(h, a, Bs, len(o), w)
        assert torch.isfinite(X).all()
        for j in (0, 20, 32):
            assert torch.equal(run(h, a, Bs[:, j:j + 1], len(o), w)[:, 0], X[:, j]), (w, j, "a column alone has other bits")
        Xn = run(h, a, Bn, len(o), w)
        assert torch.equal(Xn[:, keep], X[:, keep]), (w, "a NaN column reaches its neighbours")
    h.close()


# ------------------------------------------------------------------------------------------------
# 5.  nothing inactive is read
# ------------------------------------------------------------------------------------------------
def addressed(P, i, o):
    """Mask over the arena of what a whole solve of the handle may read: every source strip as its nv x len rectangle, every active separator's
    diagonal block as its n x n square at its leading dimension."""
    m = np.zeros(P.arena_doubles, dtype=bool)
    for q in (FWD, BWD):
        _, items, srcs = P.sparse_lists(i, o, q)
        for _, nv, s0, s1 in items:
            for a_off, ld, ln, _, _ in srcs[s0:s1]:
                l, k = np.arange(nv)[:, None], np.arange(ln)[None, :]
                m[(a_off + l + k * ld if q == FWD else a_off + k + l * ld).ravel()] = True
    heaps = ss.up(P, i) | ss.up(P, o)
    labels = {int(P.tree[h - 1]) for h in heaps}
    a_off, cols, lda, _, sep, _ = P.diag_list()
    for off, n, ld, s in zip(a_off, cols, lda, sep):
        if int(s) in labels:
            r, c = np.arange(n)[:, None], np.arange(n)[None, :]
            m[(int(off) + r + c * int(ld)).ravel()] = True
    return m


@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("which", ["A", "C", "E"])
@pytest.mark.parametrize("name", ["tree_skew", "lapl_3375x3375"])
def test_nothing_inactive_is_read(name, which, f32, inputs):
    import cholesky_amd as ca
    import torch
    I = inputs(name)
    P = I.plan
    dev, a = factored(I, f32)
    i, o, Bs, _, _ = ss.case(I, which)
    keep = addressed(P, i, o)
    assert not keep.all(), "the set prunes nothing: the test would show nothing"
    holes = a.clone()
    holes[torch.from_numpy(~keep).cuda()] = float("nan")
    h = ca.SparseSolve(dev, i, o)
    clean = run(h, a, Bs, len(o), BOTH, 3)
    got = run(h, holes, Bs, len(o), BOTH, 3)
    assert torch.isfinite(got).all() and torch.equal(got, clean), (name, which, "an element outside the lists reached the result")
    h.close()


# ------------------------------------------------------------------------------------------------
# 6.  the caller's memory
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("which", ["C", "E", "F", "G"])
def test_callers_memory(which, f32, inputs):
    import cholesky_amd as ca
    import torch
    I = inputs("tree_skew")
    dev, a = factored(I, f32)
    i, o, Bs, _, _ = ss.case(I, which)
    h = ca.SparseSolve(dev, i, o)
    fn = h.L.cholamd_sparse_solve_nrhs_f32 if f32 else h.L.cholamd_sparse_solve_nrhs
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for w in (BOTH, FWD, BWD):
        want = run(h, a, Bs, len(o), w)
        for k in (1, 33):
            gb = Guarded(len(i), ss.KMAX, len(i) + 3, values=np.array(Bs))
            gx = Guarded(len(o), ss.KMAX, len(o) + 3, values=np.full((len(o), ss.KMAX), -7.25))
            snap = gb.snapshot()
            assert fn(h.h, p(a), p(gb), len(i) + 3, p(gx), len(o) + 3, k, w, None) == 0
            dev.sync()
            gb.assert_unchanged(snap, f"set {which} which={w} nrhs={k}: Bs")
            gx.assert_guards(f"set {which} which={w} nrhs={k}: Xs")
            assert torch.equal(gx.t[:, :k], want[:, :k]) and (gx.t[:, k:] == -7.25).all(), (which, w, k, "columns past nrhs were written, or other bits")
        if len(i) == len(o):   # in place
            g = Guarded(len(i), ss.KMAX, len(i) + 3, values=np.array(Bs))
            assert fn(h.h, p(a), p(g), len(i) + 3, p(g), len(i) + 3, ss.KMAX, w, None) == 0
            dev.sync()
            g.assert_guards(f"set {which} which={w}: in place")
            assert torch.equal(g.t, want), (which, w, "in place: other bits")
    h.close()


# ------------------------------------------------------------------------------------------------
# 7.  inverse_block
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
def test_inverse_block(f32, inputs):
    import cholesky_amd as ca
    I = inputs("tree_tiny")
    P = I.plan
    dev, a = factored(I, f32)
    u = U32 if f32 else U64
    S = np.asarray(P.perm[[0, P.n // 4, P.n // 2, (3 * P.n) // 4, P.n - 1]], dtype=np.int64)     # five dofs spread over the tree: a leaf ... the root
    assert len(ss.up(P, S)) > P.levels
    h = ca.SparseSolve(dev, S, S)
    Z = h.inverse_block(a)
    dev.sync()
    Z = Z.cpu().numpy()
    A, _, _, _ = ss.dense_a(I)
    Ainv = np.linalg.inv(A)
    gate = ss.tol_forward(I, u)
    for j, dof in enumerate(S):                       # column j solves e_dof: the measure of the accuracy test with xref = column dof of A^-1
        err = ss.out_error(I, S, Z[:, j], Ainv[:, dof])
        print(f"inverse_block column {j}: error {err:.3e} (gate {gate:.3e})")
        assert err <= gate
    sym = np.abs(I.s[S, None] * (Z - Z.T) * I.s[None, S]).max() / np.abs(I.s[:, None] * Ainv * I.s[None, :]).max()
    print(f"inverse_block symmetry: {sym:.3e} (gate {2 * gate:.3e})")
    assert sym <= 2 * gate
    with pytest.raises(ValueError):
        ca.SparseSolve(dev, S, S[::-1].copy()).inverse_block(a)
    h.close()


# ------------------------------------------------------------------------------------------------
# 8.  a caller-owned stream
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["E", "G"])
def test_same_bits_on_a_callers_stream(which, inputs):
    """Everything -- the tensors, the handle's first call -- on s = torch.cuda.Stream() (non-blocking: it does not wait for the null stream), synchronised
    through s alone, against the same call on the null stream."""
    import cholesky_amd as ca
    import torch
    I = inputs("tree_skew")
    dev, a = factored(I, False)
    i, o, Bs, _, _ = ss.case(I, which)
    h = ca.SparseSolve(dev, i, o)
    want = run(h, a, Bs, len(o), BOTH, 3)
    h.close()
    torch.cuda.synchronize()
    dev2 = ca.Device(I.plan, 0)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        gb = Guarded(len(i), ss.KMAX, len(i) + 3, values=np.array(Bs))
        gx = Guarded(len(o), ss.KMAX, len(o) + 3)
        h2 = ca.SparseSolve(dev2, i, o)
        h2.solve_nrhs(a, gb.t, gx.t, BOTH, stream=s)
        s.synchronize()
        gx.assert_guards("Xs on the caller's stream")
        assert torch.equal(gx.t, want)
    h2.close()


# ------------------------------------------------------------------------------------------------
# 9.  refusals
# ------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused(inputs):
    import cholesky_amd as ca
    import torch
    I = inputs("tree_tiny")
    P = I.plan
    dev, a = factored(I, False)
    L = dev.L
    n = P.n
    msg = lambda: L.cholamd_last_error().decode()  # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ind, outd = np.array([0, 3], dtype=np.int32), np.array([1, 2, 4], dtype=np.int32)
    pi, po = ind.ctypes.data, outd.ctypes.data
    out = C.c_void_p()
    create = L.cholamd_sparse_create
    assert create(None, pi, 2, po, 3, C.byref(out)) == -4 and "NULL device" in msg()
    assert create(dev.h, pi, 2, po, 3, None) == -4 and "NULL out" in msg()
    assert create(dev.h, None, 2, po, 3, C.byref(out)) == -4 and "NULL in_dofs" in msg()
    assert create(dev.h, pi, 2, None, 3, C.byref(out)) == -4 and "NULL out_dofs" in msg()
    assert create(dev.h, pi, 0, po, 3, C.byref(out)) == -4 and "n_in = 0 < 1" in msg()
    assert create(dev.h, pi, 2, po, -1, C.byref(out)) == -4 and "n_out = -1 < 1" in msg()
    bad = np.array([0, n], dtype=np.int32)
    assert create(dev.h, bad.ctypes.data, 2, po, 3, C.byref(out)) == -4 and f"in_dofs[1] = {n} is not a dof" in msg()
    dup = np.array([1, 2, 1], dtype=np.int32)
    assert create(dev.h, pi, 2, dup.ctypes.data, 3, C.byref(out)) == -4 and "out_dofs[2] = 1 is a duplicate" in msg()
    assert not out.value
    part = ca.Device(P, 0)
    part.set_partition(1, 2)
    assert create(part.h, pi, 2, po, 3, C.byref(out)) == -4 and "complete factor" in msg() and not out.value
    h = ca.SparseSolve(dev, ind, outd)
    B, X = block(np.ones((2, 3))), block(np.zeros((3, 3)), 0, fill=-7.25)
    f = L.cholamd_sparse_solve_nrhs
    assert f(None, p(a), p(B), 2, p(X), 3, 3, -1, None) == -4 and "NULL object" in msg()
    assert f(h.h, None, p(B), 2, p(X), 3, 3, -1, None) == -4 and "NULL arena" in msg()
    assert f(h.h, p(a), None, 2, p(X), 3, 3, -1, None) == -4 and "NULL Bs" in msg()
    assert f(h.h, p(a), p(B), 2, None, 3, 3, -1, None) == -4 and "NULL Xs" in msg()
    assert f(h.h, p(a), p(B), 1, p(X), 3, 3, -1, None) == -4 and "ldb = 1" in msg()
    assert f(h.h, p(a), p(B), 2, p(X), 2, 3, -1, None) == -4 and "ldx = 2" in msg()
    assert f(h.h, p(a), p(B), 2, p(X), 3, -1, -1, None) == -4 and "nrhs = -1" in msg()
    for which in (2, -2):
        assert f(h.h, p(a), p(B), 2, p(X), 3, 3, which, None) == -4 and "which" in msg()
    assert f(h.h, p(a), p(X), 3, p(X), 3, 3, -1, None) == -4 and "aliases" in msg()         # in place needs n_in == n_out
    assert L.cholamd_sparse_counts(h.h, None) == -4 and L.cholamd_sparse_counts(None, None) == -4
    assert f(h.h, None, None, 2, None, 3, 0, -1, None) == 0                                  # nrhs = 0: accepted, nothing touched
    dev.sync()
    assert (X == -7.25).all() and (B == 1.0).all()
    # a handle whose device object became another rank of a partition afterwards
    part2 = ca.Device(P, 0)
    hp = ca.SparseSolve(part2, ind, outd)
    part2.set_partition(1, 2)
    assert f(hp.h, p(a), p(B), 2, p(X), 3, 3, -1, None) == -4 and "complete factor" in msg()
    part2.sync()
    assert (X == -7.25).all()
    with pytest.raises(ValueError):
        h.solve_nrhs(a, torch.ones(2, 3, dtype=torch.float64, device="cuda"), X)            # row-major Bs
    hp.close()
    h.close()
