"""The 64 x 64 macro-tile update kernels (k_update_mt, k32_update_mt) on trees, tile edges and deep trees (CHOLAMD_POISON=1, guarded arenas).

The level schedule takes these kernels from mt_min_tiles = 8192 sub-tiles a phase, which no small input reaches: every case here factors under
{"program": 0, "mt_min_tiles": 1, "merge_targets": 0 | 1}, fp64 and fp32, next to a device at the default options.  tests/update_mt_cases.py
names the cases and tests/test_update_mt_host.py shows on the CPU what their lists hold: tiles of one valid row or column, full tiles, SYRK
tiles on and off the diagonal, sources shorter than a 16-deep chunk (the LDS ring gets nothing), of whole chunks and of one column over, odd
operand origins, and on tree_deep tasks of 32, 33 .. 63 and 64 sources (the ring's restart between batches of 32 source descriptors).

Every factor is held to the checks of tests/test_gpu_trees.py: info (0, 0), the guards intact, the oracle's zero pattern entry for entry (fp64),
row error and reconstruction within spd_inputs' tol_factor(u) / tol_reconstruction(u) against dense numpy and the CPU oracle, u = 2^-53 or 2^-24
by the arena.  Merged, unmerged and default-path factors sum in different orders: they are compared at tol_factor(u), not bit for bit.  One
solve and the block solves of 1 and 33 columns follow on the merged macro-tile factor, and refinement on the fp32 one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tree_inputs as ti  # noqa: E402
import update_mt_cases as mc  # noqa: E402
from guarded import Guarded  # noqa: E402
from spd_inputs import U32, U64  # noqa: E402
from test_gpu_general_spd import _dense, _diag_index  # noqa: E402
from test_gpu_poison import _factor  # noqa: E402
from test_gpu_trees import _block_refs, _check_factor, _check_refinement, _check_solves, _device  # noqa: E402


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("CHOLAMD_POISON", "1")
    for v in ("CHOLAMD_SOLVE_NO_BAND", "CHOLAMD_SOLVE_NO_INV256", "CHOLAMD_SOLVE_REFERENCE_SHAPE", "CHOLAMD_MT_MIN_TILES"):
        monkeypatch.delenv(v, raising=False)


@pytest.fixture(scope="module")
def spd(tmp_path_factory):
    return lambda name: ti.cached(tmp_path_factory, name)


def _run(S, name):
    P = S.plan
    for f32 in (False, True):                                          # the lists of this input do hold macro-tile tasks, merged and unmerged
        for m in (0, 1):
            assert mc.classes(P, 1, f32, merge=(m,))["tasks"] > 0, (name, f32, m)
    ref = _device(P, {})
    aref = _factor(ref)                                                # guarded arena; info == (0, 0); guards intact
    _check_factor(S, aref, False, (name, "default"))
    Lref = _dense(S, aref.t)
    B, Xref = _block_refs(S, 33)
    for f32 in (False, True):
        u = U32 if f32 else U64
        got = []
        for path in mc.MT_PATHS:
            dev = _device(P, path)
            a = _factor(dev, f32)
            _check_factor(S, a, f32, (name, path, f32))
            got.append(_dense(S, a.t))
            assert S.row_error(got[-1], Lref) <= S.tol_factor(u), (name, path, f32)       # vs the default path's factor
        assert S.row_error(got[0], got[1]) <= S.tol_factor(u), (name, f32)               # unmerged vs merged
        _check_solves(S, dev, a, B, Xref, u=u, what=(name, f32))
        if f32:
            _check_refinement(S, dev, a, name)


@pytest.mark.parametrize("name", mc.NAMES)
def test_sweep(name, tmp_path):
    spec, heap, s = mc.CASES[name]
    S = mc.spd(tmp_path, name)
    P = S.plan
    assert P.sep_sizes[P.tree[heap - 1] - 1] == s and P.levels == 3
    _run(S, name)


@pytest.mark.parametrize("name", ["tree_skew", "tree_top", "tree_deep"])
def test_named_trees(name, spd):
    """tree_skew, tree_top: random tile boundaries with 1-dof tiles, 1-column separators as sources, a 433-column root.  tree_deep: tasks of 32,
    33 .. 63 and 64 sources -- a kernel that lost its accumulators, its place in the ring or a source at the restart between two descriptor
    batches fails the row error here.  Measured once with both kernels' batch loops cut to one batch (the merged lists hold the long tasks): row
    error 1.7e-3 against the fp64 bound 3.8e-12; the fp32 bound on the factor, 2.05e-3, is wider than that, and it is the fp32 solve that fails
    there (forward error 2.4e-3 against 2.05e-3) -- the fp32 kernel's restart is held by a thin margin, the fp64 kernel's by nine decades."""
    S = spd(name)
    if name == "tree_deep":
        for f32 in (False, True):
            c = mc.classes(S.plan, 1, f32)
            assert c["sources_32"] > 0 and c["sources_33_63"] > 0 and c["sources_64"] > 0 and c["late_chunks"] > 0
    _run(S, name)


@pytest.mark.parametrize("heap,size,col", [(4, 257, 144), (1, 193, 112)])
def test_pivot_failure_through_the_macro_tiles(heap, size, col, spd):
    """test_gpu_trees.test_pivot_failure_at_the_thresholds' construction (A'_kk = A_kk - 1.5 L_kk^2) at the first column of the last column block of
    tree_over's 257-column leaf and of its 193-column root, with every update into that column through the macro-tile kernels: info =
    (column + 1, separator) as on every other path; afterwards the same device factors good values to (0, 0)."""
    import torch
    from scipy.linalg import lapack
    S = spd("tree_over")
    P = S.plan
    lbl = int(P.tree[heap - 1])
    off = int(P.sep_offsets[lbl - 1])
    assert P.sep_sizes[lbl - 1] == size and 0 <= col < size
    k = off + col
    host = P.fill_host()
    newv = S.PAP[k, k] - 1.5 * S.Ld[k, k] ** 2
    host[_diag_index(P, host, k)] = newv
    Ap = S.PAP.copy()
    Ap[k, k] = newv
    assert lapack.dpotrf(Ap, lower=1)[1] == k + 1
    for path in mc.MT_PATHS:
        for f32 in (False, True):
            dev = _device(P, path)
            bad = Guarded(P.arena_doubles, dtype=torch.float32 if f32 else torch.float64, values=host)
            (dev.factor_f32 if f32 else dev.factor)(bad.t)
            dev.sync()
            assert dev.info() == (col + 1, lbl), (path, f32, dev.info())
            bad.assert_guards("arena of the failed factorisation")
            _factor(dev, f32)                                          # info == (0, 0)
