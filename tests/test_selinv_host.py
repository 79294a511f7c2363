"""Host side of the selected inversion (cholamd_selinv*): the CPU model that settles the structural argument for this layout, the host view of the
gather lists against the plan's block table, the symbols and their argument errors -- no device needed.

The model (selinv_ref.model) is the recursion of chol_selinv.hip in numpy.  It takes the rows below every column block and the "stored or not"
answers from the product's host view (cholamd_plan_selinv_front), reads 0.0 where the view says -1, and works on a Z arena that starts as NaN, with L
from the CPU oracle.  If a wanted entry depended on a position the panels do not store, or on one not yet computed, the comparison with
inv(P A P^T) on the mask (L_oracle != 0 plus tril(P A P^T)) would fail: this is the test of facts 1 and 2 of DESIGN.md section 11, also for
CHOLAMD_COMPACT=0.  The bound is selinv_ref's (C_SEL (k + 1) u r_i r_j in the equilibrated matrix); the observed ratios are printed (-s) and
recorded in DESIGN.md section 11."""
import ctypes as C
import re

import numpy as np
import pytest

import selinv_ref as sr
import spd_inputs as si
from conftest import CASES

SIGNATURES = {
    "cholamd_selinv": ["cholamd_device *", "const double *", "double *", "void *"],
    "cholamd_selinv_diag": ["cholamd_device *", "const double *", "double *", "void *"],
    "cholamd_selinv_entries": ["cholamd_device *", "const double *", "double *", "int64_t", "void *"],
}


@pytest.fixture(scope="module")
def ca():
    import cholesky_amd
    return cholesky_amd


def _front_checker(plan, OFF):
    """Checks of every front the model visits: positions ascending and below the block, offsets inside the arena and inside the panel of the
    column's separator, equal to what cholamd_plan_blocks + cholamd_plan_block_tile_map give for the same position (-1 for -1)."""
    offs, sizes = plan.sep_offsets.astype(np.int64), plan.sep_sizes.astype(np.int64)
    blocks = plan.blocks
    diag = {int(b[0]): b for b in blocks if b[0] == b[1]}
    p_lo = np.array([int(diag[s + 1][7]) for s in range(plan.nsep)])
    p_hi = p_lo + np.array([int(diag[s + 1][6]) for s in range(plan.nsep)]) * sizes
    sep_of_pos = np.repeat(np.arange(plan.nsep), sizes)[np.argsort(np.repeat(offs, sizes) + np.concatenate([np.arange(w) for w in sizes]), kind="stable")]
    seen = {"fronts": 0, "missing": 0}

    def check(label, blk, c0, nb, pos, off):
        seen["fronts"] += 1
        assert 0 < nb <= plan.SELINV_BLOCK and c0 == offs[label - 1] + blk * plan.SELINV_BLOCK and c0 + nb <= offs[label - 1] + sizes[label - 1]
        if len(pos) == 0:
            return
        assert (np.diff(pos) > 0).all() and pos[0] >= c0 + nb and pos[-1] < plan.n
        assert np.array_equal(off, off.T)
        i, j = np.tril_indices(len(pos))
        o = off[i, j]
        assert np.array_equal(o, OFF[pos[i], pos[j]]), (label, blk)
        st = o >= 0
        assert (o[st] < plan.arena_doubles).all() and (o[~st] == -1).all()
        s = sep_of_pos[pos[j][st]]
        assert ((o[st] >= p_lo[s]) & (o[st] < p_hi[s])).all(), (label, blk)
        seen["missing"] += int((~st).sum())
    return check, seen


def _run_model(S, name):
    plan = S.plan
    OFF = sr.offset_map(plan)
    check, seen = _front_checker(plan, OFF)
    Za = sr.model(plan, S.Lo, OFF, check)
    Z = plan.arena_to_dense(Za)
    Zr = sr.zref(S.PAP, S.Ld)
    mask = sr.mask_of(S)
    q, left_out = sr.ratio(S, Z, Zr, mask)
    print(f"selinv model {name}: n = {S.n}, k = {S.k}, fronts = {seen['fronts']}, unstored pairs read as 0.0 = {seen['missing']}, "
          f"mask = {int(mask.sum())}, max ratio = {q:.3g} (bound C_SEL = {sr.C_SEL})")
    assert left_out == 0
    assert q <= sr.C_SEL, (name, q)
    assert seen["fronts"] == sum(plan.selinv_blocks(s) for s in range(1, plan.nsep + 1))
    return seen


@pytest.mark.parametrize("case", list(CASES))
def test_model_on_the_fixtures(case):
    _run_model(sr.Fixture(case), case)


@pytest.mark.parametrize("name", si.NAMES)
def test_model_on_general_spd_inputs(name, tmp_path_factory):
    _run_model(si.cached(tmp_path_factory, name), name)


@pytest.mark.parametrize("case", ["lapl_400x400", "lapl_3375x3375"])
def test_model_without_row_compaction(case, monkeypatch):
    monkeypatch.setenv("CHOLAMD_COMPACT", "0")
    S = sr.Fixture(case)
    assert S.plan.arena_doubles == S.plan.arena_dense_doubles
    seen = _run_model(S, case + " CHOLAMD_COMPACT=0")
    assert seen["missing"] == 0                         # every row is stored: nothing reads as "not stored"


def test_symbols_signatures_and_argument_errors(ca):
    from cholesky_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    L = ca.load()
    for name, params in SIGNATURES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in the header"
        declared = [re.sub(r"\s+", " ", re.match(r"^(.*?)\w+$", a.strip()).group(1)).strip() for a in m.group(1).split(",")]
        assert declared == params, (name, declared)
        fn = getattr(L, name)
        want = [C.c_int64 if p == "int64_t" else C.c_void_p for p in params]
        assert list(fn.argtypes) == want and fn.restype is C.c_int
    assert re.search(r"#define\s+CHOLAMD_SELINV_BLOCK\s+64\b", text) and ca.Plan.SELINV_BLOCK == 64
    assert re.search(r"#define\s+CHOLAMD_SELINV_FRONT_MAX\s+8192\b", text) and ca.Plan.SELINV_FRONT_MAX == 8192
    for meth in ("selinv", "selinv_diag", "selinv_entries"):
        assert callable(getattr(ca.Device, meth))
    # without a device object every entry point refuses with CHOLAMD_ERR_ARG and says why
    buf = np.zeros(4)
    p = buf.ctypes.data
    assert L.cholamd_selinv(None, p, p, None) == -4 and b"NULL device" in L.cholamd_last_error()
    assert L.cholamd_selinv_diag(None, p, p, None) == -4 and b"NULL device" in L.cholamd_last_error()
    assert L.cholamd_selinv_entries(None, p, p, 4, None) == -4 and b"NULL device" in L.cholamd_last_error()


def test_front_view_argument_errors(ca):
    from conftest import case_paths
    plan = ca.Plan(*case_paths("lapl_400x400")[:3])
    L = plan.L
    cols = np.zeros(2, dtype=np.int32)
    assert L.cholamd_plan_selinv_blocks(plan.h, 0) == -4 and L.cholamd_plan_selinv_blocks(plan.h, plan.nsep + 1) == -4
    assert L.cholamd_plan_selinv_front(plan.h, 0, 0, 0, cols.ctypes.data, None, None) == -4
    leaf = 1
    assert L.cholamd_plan_selinv_front(plan.h, leaf, plan.selinv_blocks(leaf), 0, cols.ctypes.data, None, None) == -4
    m = L.cholamd_plan_selinv_front(plan.h, leaf, 0, 0, cols.ctypes.data, None, None)
    assert m > 0
    pos = np.zeros(m, dtype=np.int32)
    assert L.cholamd_plan_selinv_front(plan.h, leaf, 0, m - 1, cols.ctypes.data, pos.ctypes.data, None) == -4   # no room: refused, not truncated
    assert L.cholamd_plan_selinv_front(plan.h, leaf, 0, m, cols.ctypes.data, pos.ctypes.data, None) == m
    root = int(plan.tree[0])
    c0, nb, rpos, roff = plan.selinv_front(root, plan.selinv_blocks(root) - 1)
    assert len(rpos) == 0 and roff.shape == (0, 0)      # nothing below the last block of the root


def test_without_a_gpu_no_device_object_exists_for_the_selinv_calls(ca):
    """The only form CHOLAMD_ERR_NO_DEVICE can take for these calls: they take a device object, and none can be made.  (No selinv code runs here.)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("this machine has a GPU: the no-device path cannot be reached")
    from conftest import case_paths
    plan = ca.Plan(*case_paths("lapl_9x9")[:3])
    h = C.c_void_p()
    assert plan.L.cholamd_device_create(plan.h, 0, C.byref(h)) == -5     # CHOLAMD_ERR_NO_DEVICE: no object any selinv call could take
    with pytest.raises(ca.CholamdError):
        ca.Device(plan, 0)
