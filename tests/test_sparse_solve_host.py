"""Sparse solves on the host (cholamd_plan_sparse_counts / _lists / _solve_host_nrhs): the step lists of the deterministic block solve pruned to the
separators of a few dofs and their ancestors, and their walk over a host arena -- no device needed.

Inputs and dof sets: tests/sparse_sets.py.  The arena is test_solve_det_host's: the dense fp64 Cholesky factor of P A P^T on the stored positions of the
lower triangle, NaN everywhere else; the host walk also keeps NaN in every inactive row of its block, so a read of something inactive shows as a NaN.

Gates (none measured from the code under test):
  * G and H (every dof is an output): SPD.backward_error <= tol_backward() and forward_error <= tol_forward(), as tests/test_solve_det_nrhs_host.py asks
    of the full walk; the other sets: max_out |s (x - xref)| / max_all |s xref| <= tol_forward() with xref the dense solve of the scattered b with one
    long-double correction; the Laplacian fixture at 1e-9 max(1, |xref|_max) instead, and in H against the oracle's x of its own b.
  * the lists: H gives the full lists element for element and the full counts; A, B and D activate exactly the heap path of their dof; every source's
    z_off (forward) and every item's y_off lie in an active range; for A on lapl_3375x3375 the entries read are strictly fewer than the full lists'."""
import numpy as np
import pytest

import sparse_sets as ss
from test_solve_det_host import FWD, BWD, environment, inputs  # noqa: F401  (the fixtures and the shared input cache)


@pytest.mark.parametrize("which", list(ss.SETS))
@pytest.mark.parametrize("name", ss.INPUTS)
def test_the_lists_are_the_full_ones_pruned(name, which, inputs):
    """The builder's invariants hold (it returns an error otherwise); what it kept lies in the active sets and is a subsequence of the full lists."""
    I = inputs(name)
    P = I.plan
    i, o = ss.dof_set(P, which)
    c = P.sparse_counts(i, o)
    heaps = [ss.up(P, i), ss.up(P, o)]
    assert c["forward"]["separators"] == len(heaps[0]) and c["backward"]["separators"] == len(heaps[1])
    if which in "ABD":
        depth = P.heap_of(int(np.searchsorted(P.sep_offsets, np.nonzero(P.perm == i[0])[0][0], side="right"))).bit_length() - 1
        assert len(heaps[0]) == depth + 1 and c["forward"]["separators"] == depth + 1 and c["backward"]["separators"] == depth + 1
    union = ss.active_mask(P, heaps[0] | heaps[1])
    assert c["positions"] == int(union.sum())
    assert c["ranges"] == int(np.count_nonzero(np.diff(np.concatenate([[0], union.astype(np.int8)])) == 1))
    full = P.solve_det_counts()
    for q, w in ((FWD, "forward"), (BWD, "backward")):
        act = ss.active_mask(P, heaps[q])
        steps, items, srcs = P.sparse_lists(i, o, q)
        fsteps, fitems, fsrcs = P.solve_det_lists(q)
        assert (len(steps), len(items), len(srcs)) == (c[w]["steps"], c[w]["items"], c[w]["sources"])
        assert len(steps) <= len(fsteps) and c[w]["entries"] <= full[w]["entries"]
        # every item owns active positions only; every source reads active positions only (forward: where it matters; backward: ancestors, checked too)
        for y_off, nv, _, _ in items:
            assert act[y_off:y_off + nv].all(), (name, which, w, "an item owns an inactive position")
        for _, _, ln, z_off, _ in srcs:
            assert act[z_off:z_off + ln].all(), (name, which, w, "a source reads an inactive position")
        # steps, items and sources are subsequences of the full lists, in their order
        fs = [(int(a), int(b)) for a, b in fsteps[:, :2]]
        pos = -1
        for lvl, col0 in steps[:, :2]:
            pos = fs.index((int(lvl), int(col0)), pos + 1)
        fy = fitems[:, 0].tolist()
        pos = -1
        for t in range(len(steps)):
            for y in items[steps[t, 2]:steps[t, 3], 0]:
                pos = fy.index(int(y), pos + 1)
        fsrc = {tuple(r) for r in fsrcs.tolist()}
        assert all(tuple(r) in fsrc for r in srcs.tolist())
        # the entries: the kept strips plus the active separators' own span triangles
        ent = int(sum(int(nv) * int(srcs[k, 2]) for _, nv, s0, s1 in items for k in range(s0, s1)))
        for h in heaps[q]:
            m = int(P.sep_sizes[int(P.tree[h - 1]) - 1])
            ent += sum(min(256, m - c0) * (min(256, m - c0) + 1) // 2 for c0 in range(0, m, 256))
        assert ent == c[w]["entries"]
        # a span step survives iff an active separator of its level is wider than its first column -- with or without items
        want = {(h.bit_length() - 1, c0) for h in heaps[q] for c0 in range(0, int(P.sep_sizes[int(P.tree[h - 1]) - 1]), 256)}
        assert {(int(a), int(b)) for a, b in steps[:, :2] if b >= 0} == want


@pytest.mark.parametrize("name", ss.INPUTS)
def test_everything_active_gives_the_full_lists(name, inputs):
    I = inputs(name)
    P = I.plan
    i, o = ss.dof_set(P, "H")
    c, full = P.sparse_counts(i, o), P.solve_det_counts()
    for q, w in ((FWD, "forward"), (BWD, "backward")):
        assert {k: c[w][k] for k in ("steps", "items", "sources", "entries")} == full[w]
        assert c[w]["separators"] == P.nsep
        for a, b in zip(P.sparse_lists(i, o, q), P.solve_det_lists(q)):
            assert np.array_equal(a, b), (name, w)
    assert c["positions"] == P.n and c["ranges"] == 1


def test_one_leaf_dof_reads_far_less_of_the_factor(inputs):
    I = inputs("lapl_3375x3375")
    P = I.plan
    i, o = ss.dof_set(P, "A")
    c, full = P.sparse_counts(i, o), P.solve_det_counts()
    for w in ("forward", "backward"):
        print(f"lapl_3375x3375, one leaf dof, {w}: {c[w]['entries']} of {full[w]['entries']} entries of L read "
              f"({c[w]['entries'] / full[w]['entries']:.4f}), {c[w]['steps']} of {full[w]['steps']} steps, {c[w]['separators']} of {P.nsep} separators")
        assert c[w]["entries"] < full[w]["entries"] and c[w]["separators"] == P.levels


@pytest.mark.parametrize("which", list(ss.SETS))
@pytest.mark.parametrize("name", ss.INPUTS)
def test_host_walk_matches_the_dense_solve(name, which, inputs):
    I = inputs(name)
    P = I.plan
    i, o, Bs, B, Xref = ss.case(I, which)
    for nrhs in ss.NRHS:
        pad = 3 if nrhs == 33 else 0
        X = P.sparse_solve_host_nrhs(I.arena, i, o, -1, Bs[:, :nrhs], ldb=len(i) + pad, ldx=len(o) + pad)
        assert X.shape == (len(o), nrhs)
        for j in range(nrhs):
            ss.column_gate(I, o, X[:, j], Xref[:, j], f"{name} set {which} nrhs={nrhs} column {j}")
            if which in "GH" and I.S is not None:
                be = I.S.backward_error(X[:, j], B[:, j])
                assert be <= I.S.tol_backward(), (name, which, j, be)
        if nrhs == 33:
            X33 = X
    # a column alone has the bits it has among 33; the halves compose to the solve where every dof is both input and output
    assert np.array_equal(P.sparse_solve_host_nrhs(I.arena, i, o, -1, Bs[:, 5:6])[:, 0], X33[:, 5])
    if which == "H":
        Y = P.sparse_solve_host_nrhs(I.arena, i, o, FWD, Bs)
        assert np.array_equal(P.sparse_solve_host_nrhs(I.arena, i, o, BWD, Y), X33)
        assert np.array_equal(P.solve_det_host_nrhs(I.arena, -1, B), X33), "everything active: the bits of the full host walk"
        if I.S is None:   # the fixture's own right-hand side against the oracle's x
            x = P.sparse_solve_host_nrhs(I.arena, i, o, -1, I.b[:, None])[:, 0]
            assert float(np.abs(x - I.xo).max()) <= 1e-9 * max(1.0, float(np.abs(I.xo).max()))


@pytest.mark.parametrize("which", ["A", "C", "E", "F"])
@pytest.mark.parametrize("name", ["tree_tiny", "tree_skew", "g7_ragged"])
def test_half_solves_on_the_host(name, which, inputs):
    """FORWARD: the outputs inside up(in) against the dense M^-1 b, those outside exactly +0.0.  BACKWARD: against the dense M^-T of the inputs inside
    up(out) -- an input outside it cannot reach a wanted output."""
    import scipy.linalg as sl
    I = inputs(name)
    P = I.plan
    i, o, Bs, B, _ = ss.case(I, which)
    p = np.asarray(I.perm, dtype=np.int64)
    tol = ss.tol_forward(I)
    act_fw, act_bw = ss.active_mask(P, ss.up(P, i)), ss.active_mask(P, ss.up(P, o))
    iperm = np.empty(P.n, dtype=np.int64)
    iperm[p] = np.arange(P.n)
    Y = P.sparse_solve_host_nrhs(I.arena, i, o, FWD, Bs)
    Yref = np.empty_like(B)
    Yref[p] = sl.solve_triangular(I.Ld, B[p], lower=True)
    outside = ~act_fw[iperm[o]]
    assert (Y[outside] == 0.0).all() and not np.signbit(Y[outside]).any() and (Yref[o][outside] == 0.0).all()
    # L^-1 P b = (S^-1 L)^-1 (S^-1 P b): the forward half is the equilibrated system's own, so its measure carries no scale
    assert np.abs(Y - Yref[o]).max() <= tol * np.abs(Yref).max(), (name, which, "forward")
    Bin = np.where(act_bw[iperm][:, None], B, 0.0)
    Z = P.sparse_solve_host_nrhs(I.arena, i, o, BWD, Bs)
    Zref = np.empty_like(B)
    Zref[p] = sl.solve_triangular(I.Ld, Bin[p], lower=True, trans="T")
    assert np.isfinite(Z).all()
    assert np.abs(I.s[o, None] * (Z - Zref[o])).max() <= tol * max(np.abs(I.s[:, None] * Zref).max(), np.finfo(float).tiny), (name, which, "backward")


def test_bad_arguments_are_refused(inputs):
    I = inputs("tree_tiny")
    P = I.plan
    n, k = P.n, 3
    ind, outd = np.array([0, 3], dtype=np.int32), np.array([1, 2, 4], dtype=np.int32)
    B, X = np.ones((k, 2)), np.full((k, 3), -7.0)
    f = P.L.cholamd_plan_sparse_solve_host_nrhs
    ar, b, x, pi, po = I.arena.ctypes.data, B.ctypes.data, X.ctypes.data, ind.ctypes.data, outd.ctypes.data
    err = lambda: P.L.cholamd_last_error().decode()  # noqa: E731
    for which in (2, -2):
        assert f(P.h, ar, pi, 2, po, 3, which, b, 2, x, 3, k) == -4 and "which" in err()
    assert f(None, ar, pi, 2, po, 3, -1, b, 2, x, 3, k) == -4 and "NULL plan" in err()
    assert f(P.h, None, pi, 2, po, 3, -1, b, 2, x, 3, k) == -4 and "NULL arena" in err()
    assert f(P.h, ar, None, 2, po, 3, -1, b, 2, x, 3, k) == -4 and "NULL in_dofs" in err()
    assert f(P.h, ar, pi, 2, None, 3, -1, b, 2, x, 3, k) == -4 and "NULL out_dofs" in err()
    assert f(P.h, ar, pi, 2, po, 3, -1, None, 2, x, 3, k) == -4 and "NULL Bs" in err()
    assert f(P.h, ar, pi, 2, po, 3, -1, b, 2, None, 3, k) == -4 and "NULL Xs" in err()
    assert f(P.h, ar, pi, 0, po, 3, -1, b, 2, x, 3, k) == -4 and "n_in = 0 < 1" in err()
    assert f(P.h, ar, pi, 2, po, 0, -1, b, 2, x, 3, k) == -4 and "n_out = 0 < 1" in err()
    assert f(P.h, ar, pi, 2, po, 3, -1, b, 1, x, 3, k) == -4 and "ldb = 1" in err()
    assert f(P.h, ar, pi, 2, po, 3, -1, b, 2, x, 2, k) == -4 and "ldx = 2" in err()
    assert f(P.h, ar, pi, 2, po, 3, -1, b, 2, x, 3, -1) == -4 and "nrhs = -1" in err()
    bad = np.array([0, n], dtype=np.int32)
    assert f(P.h, ar, bad.ctypes.data, 2, po, 3, -1, b, 2, x, 3, k) == -4 and f"in_dofs[1] = {n} is not a dof" in err()
    bad = np.array([1, -1, 4], dtype=np.int32)
    assert f(P.h, ar, pi, 2, bad.ctypes.data, 3, -1, b, 2, x, 3, k) == -4 and "out_dofs[1] = -1 is not a dof" in err()
    dup = np.array([1, 2, 1], dtype=np.int32)
    assert f(P.h, ar, pi, 2, dup.ctypes.data, 3, -1, b, 2, x, 3, k) == -4 and "out_dofs[2] = 1 is a duplicate" in err()
    dup = np.array([3, 3], dtype=np.int32)
    assert f(P.h, ar, dup.ctypes.data, 2, po, 3, -1, b, 2, x, 3, k) == -4 and "in_dofs[1] = 3 is a duplicate" in err()
    out = np.zeros(12, dtype=np.int64)
    assert P.L.cholamd_plan_sparse_counts(P.h, dup.ctypes.data, 2, po, 3, out.ctypes.data) == -4 and "duplicate" in err()
    assert P.L.cholamd_plan_sparse_counts(P.h, pi, 2, po, 3, None) == -4
    assert P.L.cholamd_plan_sparse_lists(P.h, pi, 2, po, 3, -1, out.ctypes.data, out.ctypes.data, out.ctypes.data) == -4 and "which" in err()
    assert (X == -7.0).all() and (B == 1.0).all()
    # the same dof in both lists is fine; nrhs = 0: accepted, nothing is read or written
    assert f(P.h, ar, pi, 2, pi, 2, -1, b, 2, x, 3, k) == 0
    X[:] = -7.0
    assert f(P.h, None, pi, 2, po, 3, 0, None, 2, None, 3, 0) == 0
    assert (X == -7.0).all() and (B == 1.0).all()


def test_the_library_has_the_entry_points():
    import cholesky_amd as ca
    L = ca.load()
    for f in ("cholamd_plan_sparse_solve_host_nrhs", "cholamd_plan_sparse_counts", "cholamd_plan_sparse_lists", "cholamd_sparse_create", "cholamd_sparse_destroy",
              "cholamd_sparse_counts", "cholamd_sparse_solve_nrhs", "cholamd_sparse_solve_nrhs_f32"):
        assert hasattr(L, f), f
    assert ca.SparseSolve is not None
