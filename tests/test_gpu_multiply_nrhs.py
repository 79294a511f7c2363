"""Block products with the factor on the device: Y = M Z, M^T Z and M M^T Z for many columns (cholamd_multiply_half_nrhs*, cholamd_multiply_nrhs*).

The device option "multiply_nrhs_min" picks the path of a chunk of 32 columns: 1 = every chunk takes the block kernel (k_multiply_nrhs), 33 = every chunk
goes column by column through the single-vector products, 0 = the measured default.  No test depends on the default's value.

Gates -- those of tests/multiply_ref.py and tests/test_gpu_multiply.py, derived, none measured from the code under test; u = 2^-53 in the products (their
arithmetic is fp64 for either factor):
 1. per column against the device's own factor (downloaded, tril of its image, an fp32 factor converted to fp64): componentwise (k + 2) u |L| |z|, the
    inner-product bound, k = the most non-zero terms of a component.  The bound holds for ANY summation order, so the four partial tiles of a workgroup
    and the fused multiply-adds of the MFMA need no wider gate than the single-vector kernel.
 3. round trip solve_half_nrhs(w)(multiply_half_nrhs(w)(Z)) against Z: tol_forward(u) = C_FE (k + 1) u kappa with u of the FACTOR, in the measures of
    test_gpu_multiply (FORWARD: max-norm relative, BACKWARD: SPD.forward_error).
 4. multiply_nrhs against A Z: |y - A z| <= C_BE (k + 1) u |L| |L^T| |z| componentwise, u of the factor.

Size constants of the new kernel (chol_plan.h, chol_multiply_nrhs.hip), each swept one below, at and one above as a separator size at a leaf, a middle
separator and the root:
   16  CHOL_MUL_TILE: the positions of an item, the lines of an MFMA tile
   32  CHOL_MULN_KSTEP: the reduction steps of one chunk -- the 8 MFMA steps whose loads are in flight together, and the unit a wave takes at a time
  128  CHOL_MULN_WAVES * CHOL_MULN_KSTEP: one round of chunks over the four waves, i.e. the reduction length from which every wave has a share and the
       first wave gets a second chunk

Every test prints its largest error / gate ratio with pytest -s; DESIGN.md section 13 records them."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import multiply_ref as mr  # noqa: E402
import spd_inputs as si  # noqa: E402
import tree_inputs  # noqa: E402
from conftest import CASES, ROOT, case_paths  # noqa: E402
from guarded import Guarded  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from spd_inputs import C_BE, U32, U64  # noqa: E402

FWD, BWD = 0, 1
BLOCK, COLUMNS, DEFAULT = 1, 33, 0         # values of the option multiply_nrhs_min
PRECISIONS = [False, True]
PIDS = ["fp64", "fp32"]
NRHS = [1, 15, 16, 17, 31, 32, 33, 70]
NRHS_OF = {"lapl_9x9": NRHS, "lapl_25x25": NRHS, "lapl_400x400": NRHS, "lapl_3375x3375": [32, 70]}
TREE_NAMES = tree_inputs.NAMED + tree_inputs.SINGLE
SWEEP = [15, 16, 17, 31, 32, 33, 127, 128, 129]
FULL_INPUTS = ["lapl_25x25", "lapl_3375x3375", "lapl_3375_scaled", "g7_ragged", "tree_over", "tree_skew"]
POISON_INPUTS = ["lapl_400x400", "tree_over"]


@pytest.fixture(scope="module")
def ca():
    import cholesky_amd
    orc.use_own_kernels()
    return cholesky_amd


@pytest.fixture(scope="module")
def spd(tmp_path_factory):
    return lambda name: tree_inputs.cached(tmp_path_factory, name)


def block(V, ld=None):
    """An n x k Guarded block holding V (column-major, leading dimension ld, default n + 3)."""
    return Guarded(V.shape[0], V.shape[1], V.shape[0] + 3 if ld is None else ld, values=V)


def empty_block(n, k, ld=None):
    return Guarded(n, k, n + 3 if ld is None else ld)


def cuda(v):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).cuda()


def factored(ca, plan, f32):
    dev = ca.Device(plan, 0)
    a = dev.new_arena_f32() if f32 else dev.new_arena()
    (dev.fill_f32 if f32 else dev.fill)(a)
    (dev.factor_f32 if f32 else dev.factor)(a)
    dev.sync()
    assert dev.info() == (0, 0)
    return dev, a


_DEV, _REF = {}, {}


def device_of(ca, key, plan, f32):
    """(dev, arena, tril of the arena's image as CSR) of a factored plan, cached; the option is left at BLOCK by whoever changes it."""
    if (key, f32) not in _DEV:
        dev, a = factored(ca, plan, f32)
        _DEV[key, f32] = (dev, a, si.arena_to_sparse(plan, a.cpu().numpy().astype(np.float64)))
    return _DEV[key, f32]


def references(Dsp, perm, Z):
    """Gate 1's reference of every column of Z for both halves: {which: (Yref, |L| |Z|, k)}."""
    out = {}
    for which in (FWD, BWD):
        cols = [mr.product_sparse(Dsp, perm, Z[:, j], which) for j in range(Z.shape[1])]
        out[which] = (np.stack([c[0] for c in cols], axis=1), np.stack([c[1] for c in cols], axis=1), max(c[2] for c in cols))
    return out


def reference(key, f32, Dsp, perm, Z):
    """references() once per (input, precision)."""
    if (key, f32) not in _REF:
        _REF[key, f32] = references(Dsp, perm, Z)
    return _REF[key, f32]


def gate1(Y, ref, which, tag):
    Yref, absprod, k = ref[which]
    worst = 0.0
    for j in range(Y.shape[1]):
        r = mr.gate_ratio(Y[:, j], Yref[:, j], absprod[:, j], k)
        assert r <= 1.0, (tag, which, j, r)
        worst = max(worst, r)
    return worst


def half_block(dev, arena, Z, which, tag=""):
    """multiply_half_nrhs into a guarded block (ld = n + 3) from a guarded Z (ld = n + 5) that must come back unchanged; then in place: the same bits."""
    n, k = Z.shape
    Zg, Yg = block(Z, n + 5), empty_block(n, k)
    snap = Zg.snapshot()
    dev.multiply_half_nrhs(arena, Zg.t, Yg.t, which)
    dev.sync()
    Zg.assert_unchanged(snap, f"{tag}: Z")
    Yg.assert_guards(f"{tag}: Y")
    Y = Yg.numpy()
    Zi = block(Z)
    dev.multiply_half_nrhs(arena, Zi.t, Zi.t, which)
    dev.sync()
    Zi.assert_guards(f"{tag}: in place")
    assert np.array_equal(Zi.numpy(), Y), f"{tag}: in place returns other bits"
    return Y


def plain_plan(ca, name):
    return ca.Plan(*case_paths(name)[:3])


# ------------------------------------------------------------------------------------------------
# 1. the block path against the device's own factor
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("name", list(NRHS_OF))
def test_block_path_matches_the_downloaded_factor(name, f32, ca):
    plan = plain_plan(ca, name)
    dev, arena, Dsp = device_of(ca, name, plan, f32)
    dev.set_option("multiply_nrhs_min", BLOCK)
    Z = np.random.default_rng(41).standard_normal((plan.n, max(NRHS)))
    ref = reference(name, f32, Dsp, plan.perm, Z)
    worst = 0.0
    for k in NRHS_OF[name]:
        for which in (FWD, BWD):
            Y = half_block(dev, arena, Z[:, :k], which, f"{name} {PIDS[f32]} nrhs={k} which={which}")
            worst = max(worst, gate1(Y, ref, which, (name, k)))
    print(f"{name} {PIDS[f32]} block path: largest error / gate = {worst:.3f}")


# ------------------------------------------------------------------------------------------------
# 2. the column path is the single-vector product; the default path
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
def test_column_path_is_the_single_product_and_default_path(f32, ca):
    import torch
    name, k = "lapl_400x400", 35                  # a whole chunk and a tail of three columns
    plan = plain_plan(ca, name)
    n = plan.n
    dev, arena, Dsp = device_of(ca, name, plan, f32)
    Z = np.random.default_rng(41).standard_normal((n, max(NRHS)))   # (the block of test 1: the same reference)
    ref = reference(name, f32, Dsp, plan.perm, Z)
    try:
        dev.set_option("multiply_nrhs_min", COLUMNS)
        for which in (FWD, BWD):
            Y = half_block(dev, arena, Z[:, :k], which, f"column path which={which}")
            for j in range(k):
                y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
                dev.multiply_half(arena, cuda(Z[:, j]), y, which)
                dev.sync()
                assert np.array_equal(y.cpu().numpy(), Y[:, j]), (which, j)
        dev.set_option("multiply_nrhs_min", DEFAULT)
        for which in (FWD, BWD):
            r = gate1(half_block(dev, arena, Z[:, :k], which, f"default path which={which}"), ref, which, "default")
            print(f"{name} {PIDS[f32]} default path which={which}: error / gate = {r:.3f}")
    finally:
        dev.set_option("multiply_nrhs_min", BLOCK)


# ------------------------------------------------------------------------------------------------
# 3. the full product: FORWARD of BACKWARD bit for bit, and gate 4 against A Z
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("name", FULL_INPUTS)
def test_full_product(name, f32, ca, spd):
    S = spd(name)
    n, k = S.n, 35
    dev, arena, Dsp = device_of(ca, "spd:" + name, S.plan, f32)
    u = U32 if f32 else U64
    Z = np.random.default_rng(42).standard_normal((n, k)) / S.s[:, None]
    AZ = S.A_sparse @ Z
    aD = abs(Dsp)
    bound = np.empty_like(Z)
    bound[S.perm] = C_BE * (S.k + 1) * u * (aD @ (aD.T @ np.abs(Z[S.perm])))
    try:
        for setting in (BLOCK, COLUMNS, DEFAULT):
            dev.set_option("multiply_nrhs_min", setting)
            Zg, Wg, Yg, Fg = block(Z, n + 5), empty_block(n, k), empty_block(n, k), empty_block(n, k)
            snap = Zg.snapshot()
            dev.multiply_nrhs(arena, Zg.t, Fg.t)
            dev.multiply_half_nrhs(arena, Zg.t, Wg.t, BWD)
            dev.multiply_half_nrhs(arena, Wg.t, Yg.t, FWD)
            dev.sync()
            Zg.assert_unchanged(snap, "Z")
            Fg.assert_guards("the full product")
            F = Fg.numpy()
            assert np.array_equal(F, Yg.numpy()), f"setting {setting}: multiply_nrhs is not FORWARD of BACKWARD"
            assert np.isfinite(F).all()
            r = float((np.abs(F - AZ) / bound).max())
            print(f"{name} {PIDS[f32]} setting {setting}: M M^T Z against A Z, error / gate = {r:.3e}")
            assert r <= 1.0
            Zi = block(Z)
            dev.multiply_nrhs(arena, Zi.t, Zi.t)
            dev.sync()
            Zi.assert_guards("in place")
            assert np.array_equal(Zi.numpy(), F), "in place: the same bits"
    finally:
        dev.set_option("multiply_nrhs_min", BLOCK)


# ------------------------------------------------------------------------------------------------
# 4. determinism
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("name", ["lapl_3375x3375", "tree_over"])
def test_two_calls_return_the_same_bits(name, f32, ca, spd):
    S = spd(name)
    dev, arena, _ = device_of(ca, "spd:" + name, S.plan, f32)
    dev.set_option("multiply_nrhs_min", BLOCK)
    n, k = S.n, 33
    Zg = block(np.random.default_rng(43).standard_normal((n, k)))
    outs = []
    for _ in range(2):
        o = [empty_block(n, k) for _ in range(3)]
        dev.multiply_half_nrhs(arena, Zg.t, o[0].t, FWD)
        dev.multiply_half_nrhs(arena, Zg.t, o[1].t, BWD)
        dev.multiply_nrhs(arena, Zg.t, o[2].t)
        dev.sync()
        outs.append([g.numpy() for g in o])
    for a, b in zip(*outs):
        assert np.isfinite(a).all() and np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------
# 5. column isolation
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("name", ["lapl_400x400", "tree_over"])
def test_columns_are_isolated(name, f32, ca, spd):
    S = spd(name)
    dev, arena, _ = device_of(ca, "spd:" + name, S.plan, f32)
    dev.set_option("multiply_nrhs_min", BLOCK)
    n, k = S.n, 20
    Z = np.random.default_rng(44).standard_normal((n, k))
    Z[:, 11] = 0.0
    Zbad = Z.copy()
    Zbad[:, 3] = np.nan
    Zbad[n // 2, 7] = np.inf
    others = [j for j in range(k) if j not in (3, 7)]

    def run(V):
        o = [empty_block(n, k) for _ in range(3)]
        Vg = block(V)
        dev.multiply_half_nrhs(arena, Vg.t, o[0].t, FWD)
        dev.multiply_half_nrhs(arena, Vg.t, o[1].t, BWD)
        dev.multiply_nrhs(arena, Vg.t, o[2].t)
        dev.sync()
        for g in o:
            g.assert_guards(name)
        return [g.numpy() for g in o]

    for good, bad in zip(run(Z), run(Zbad)):
        assert np.isfinite(good).all()
        assert np.array_equal(good[:, others], bad[:, others]), "a NaN / inf column reached another column"
        assert (good[:, 11] == 0.0).all() and (bad[:, 11] == 0.0).all(), "an all-zero column gives zeros"
        assert np.isnan(bad[:, 3]).all()
        assert not np.isfinite(bad[:, 7]).all()


# ------------------------------------------------------------------------------------------------
# 6. trees, and the kernel's size constants
# ------------------------------------------------------------------------------------------------
def tree_ratio(dev, arena, Dsp, perm, Z, tag):
    dev.set_option("multiply_nrhs_min", BLOCK)
    ref = references(Dsp, perm, Z)
    worst = 0.0
    for which in (FWD, BWD):
        worst = max(worst, gate1(half_block(dev, arena, Z, which, f"{tag} which={which}"), ref, which, tag))
    print(f"{tag}: largest error / gate = {worst:.3f}")
    return worst


@pytest.mark.parametrize("name", TREE_NAMES)
def test_block_products_on_trees(name, ca, spd):
    S = spd(name)
    Z = np.random.default_rng(45).standard_normal((S.n, 17))
    for f32 in PRECISIONS:
        dev, arena, Dsp = device_of(ca, "spd:" + name, S.plan, f32)
        tree_ratio(dev, arena, Dsp, S.perm, Z, f"{name} {PIDS[f32]}")


@pytest.mark.parametrize("s", SWEEP)
@pytest.mark.parametrize("position", ["leaf", "middle", "root"])
def test_block_products_at_kernel_size_constants(position, s, ca, tmp_path):
    S = tree_inputs.sweep(tmp_path, position, s, leaf=("band", 20) if position == "leaf" and s > 32 else "dense", oracle=False)
    Z = np.random.default_rng(46).standard_normal((S.n, 17))
    for f32 in PRECISIONS:
        dev, a = factored(ca, S.plan, f32)
        Dsp = si.arena_to_sparse(S.plan, a.cpu().numpy().astype(np.float64))
        tree_ratio(dev, a, Dsp, S.perm, Z, f"sweep {position} {s} {PIDS[f32]}")


# ------------------------------------------------------------------------------------------------
# 7. poison: a fresh child process per setting, the same uploaded arena, the same bits
# ------------------------------------------------------------------------------------------------
def poison_child():
    """Both halves and the full product of POISON_INPUTS, 20 columns, block and default path, on an arena uploaded from the host (the dense factor on the
    lower triangle, NaN elsewhere), printed as hex words: the parent compares the output of a poisoned and an unpoisoned child."""
    import cholesky_amd as ca
    import torch
    with tempfile.TemporaryDirectory() as tmp:
        for name in POISON_INPUTS:
            if name in CASES:
                plan = ca.Plan(*case_paths(name)[:3])
            else:
                spec = tree_inputs.TREES[name]
                plan = si.SPD(tmp, spec, 3000 + spec["seed"], name=name, oracle=False, dense=False).plan
            n, k = plan.n, 20
            D = plan.arena_to_dense(plan.fill_host())
            host = mr.arena_from_lower(plan, np.linalg.cholesky(np.tril(D) + np.tril(D, -1).T))
            assert np.isnan(host).any()
            Z = np.random.default_rng(47).standard_normal((n, k))
            for f32 in PRECISIONS:
                dev = ca.Device(plan, 0)
                arena = torch.from_numpy(host.astype(np.float32) if f32 else host).cuda()
                for setting in (BLOCK, DEFAULT):
                    dev.set_option("multiply_nrhs_min", setting)
                    Zg = block(Z)
                    o = [empty_block(n, k) for _ in range(3)]
                    dev.multiply_half_nrhs(arena, Zg.t, o[0].t, FWD)
                    dev.multiply_half_nrhs(arena, Zg.t, o[1].t, BWD)
                    dev.multiply_nrhs(arena, Zg.t, o[2].t)
                    dev.sync()
                    for tag, g in zip(("forward", "backward", "full"), o):
                        g.assert_guards(tag)
                        v = g.numpy()
                        assert np.isfinite(v).all(), (name, f32, setting, tag)
                        print(name, PIDS[f32], setting, tag, np.ascontiguousarray(v.T).view(np.uint64).tobytes().hex())
    print("poison child: ok")


def test_poisoned_buffers_change_nothing():
    outs = []
    for poison in ("0", "1"):
        env = dict(os.environ, CHOLAMD_POISON=poison)
        for v in ("CHOLAMD_SOLVE_NO_BAND", "CHOLAMD_COMPACT", "CHOLAMD_MULTIPLY_NRHS_MIN"):
            env.pop(v, None)
        p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and "poison child: ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
        outs.append(p.stdout)
    assert outs[0].count("\n") == 3 * 2 * 2 * len(POISON_INPUTS) + 1
    assert outs[0] == outs[1], "the poisoned run returns other bits"


# ------------------------------------------------------------------------------------------------
# 8. arguments
# ------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_untouched(ca):
    import torch
    plan = plain_plan(ca, "lapl_400x400")
    n, k = plan.n, 3
    V = np.random.default_rng(48).standard_normal((n, k))
    msg = lambda: ca.load().cholamd_last_error().decode()  # noqa: E731
    for f32 in PRECISIONS:
        dev, arena, _ = device_of(ca, "lapl_400x400", plan, f32)
        L, h = dev.L, dev.h
        sfx = "_f32" if f32 else ""
        half, full = getattr(L, "cholamd_multiply_half_nrhs" + sfx), getattr(L, "cholamd_multiply_nrhs" + sfx)
        Zg, Yg = block(V, n), empty_block(n, k, n)
        A, Z, Y = arena.data_ptr(), Zg.data_ptr(), Yg.data_ptr()     # (plain integers: ctypes takes them for void *)
        snap = Zg.snapshot()
        for setting in (BLOCK, COLUMNS):
            dev.set_option("multiply_nrhs_min", setting)
            assert half(h, A, Z, n, Y, n, k, 2, None) == -4 and "which" in msg()
            assert half(h, A, Z, n, Y, n, k, -1, None) == -4 and "which" in msg()
            assert half(h, A, Z, n, Y, n, -1, FWD, None) == -4 and "nrhs" in msg()
            assert full(h, A, Z, n, Y, n, -1, None) == -4 and "nrhs" in msg()
            assert half(h, A, Z, n - 1, Y, n, k, FWD, None) == -4 and "leading" in msg()
            assert half(h, A, Z, n, Y, n - 1, k, BWD, None) == -4 and "leading" in msg()
            assert full(h, A, Z, n - 1, Y, n, k, None) == -4 and full(h, A, Z, n, Y, n - 1, k, None) == -4
            assert half(h, None, Z, n, Y, n, k, FWD, None) == -4 and "NULL" in msg()
            assert half(h, A, None, n, Y, n, k, FWD, None) == -4 and half(h, A, Z, n, None, n, k, BWD, None) == -4
            assert full(h, None, Z, n, Y, n, k, None) == -4 and full(h, A, None, n, Y, n, k, None) == -4 and full(h, A, Z, n, None, n, k, None) == -4
            assert half(None, A, Z, n, Y, n, k, FWD, None) == -4 and full(None, A, Z, n, Y, n, k, None) == -4
            # nrhs == 0 returns 0 and touches nothing, whatever the pointers
            assert half(h, A, Z, n, Y, n, 0, FWD, None) == 0 and full(h, A, Z, n, Y, n, 0, None) == 0
            assert half(h, None, None, n, None, n, 0, BWD, None) == 0 and full(h, None, None, n, None, n, 0, None) == 0
            # a result inside the arena, and one whose LAST column reaches into it
            before = arena.clone()
            inside = A + 16 * arena.element_size()
            assert half(h, A, Z, n, inside, n, k, FWD, None) == -4 and "overlaps" in msg()
            assert full(h, A, Z, n, inside, n, k, None) == -4 and "overlaps" in msg()
            if Y < A:
                reach = (A - Y) // 8 + 8           # a leading dimension that puts column 1 of Y inside the arena
                if reach >= n:
                    assert half(h, A, Z, n, Y, reach, 2, BWD, None) == -4 and "overlaps" in msg()
                    assert full(h, A, Z, n, Y, reach, 2, None) == -4 and "overlaps" in msg()
            dev.sync()
            assert torch.equal(torch.nan_to_num(arena), torch.nan_to_num(before))
        with pytest.raises(ca.CholamdError, match="which"):
            dev.multiply_half_nrhs(arena, Zg.t, Yg.t, 2)
        with pytest.raises(ValueError):
            dev.multiply_half_nrhs(arena, Zg.t[:-1], Yg.t, FWD)
        with pytest.raises(ValueError):
            dev.multiply_nrhs(arena, Zg.t, Yg.t[:, :-1])
        with pytest.raises(ValueError):
            dev.multiply_nrhs(arena, Zg.t, Yg.t.float())
        # another rank of a partitioned object holds no complete factor
        part = ca.Device(plan, 0)
        part.set_partition(1, 2)
        for setting in (BLOCK, COLUMNS):
            part.set_option("multiply_nrhs_min", setting)
            assert half(part.h, A, Z, n, Y, n, k, FWD, None) == -4 and "complete factor" in msg()
            assert full(part.h, A, Z, n, Y, n, k, None) == -4 and "complete factor" in msg()
        part.sync()
        dev.sync()
        Yg.assert_guards("Y")
        assert (Yg.bits() == Yg.pattern).all(), "a refused call wrote Y"
        Zg.assert_unchanged(snap, "Z")
        dev.set_option("multiply_nrhs_min", BLOCK)


# ------------------------------------------------------------------------------------------------
# 9. later calls allocate nothing
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
def test_later_calls_allocate_nothing(f32, ca):
    plan = plain_plan(ca, "lapl_400x400")
    n, k = plan.n, 40
    dev, arena = factored(ca, plan, f32)
    live = ca.load().cholamd_debug_live_buffers
    Zg, Yg = block(np.random.default_rng(49).standard_normal((n, k))), empty_block(n, k)
    dev.set_option("multiply_nrhs_min", COLUMNS)       # the lists and the vectors of the single products, no block yet
    dev.multiply_nrhs(arena, Zg.t, Yg.t)
    dev.sync()
    base = live()
    dev.set_option("multiply_nrhs_min", BLOCK)
    counts = []
    for i in range(3):
        dev.multiply_half_nrhs(arena, Zg.t, Yg.t, i % 2)
        dev.multiply_nrhs(arena, Zg.t, Yg.t)
        dev.sync()
        counts.append(live())
    assert counts[0] == base + 2, "the two n x 32 blocks are allocated at the first block call"
    assert counts[2] == counts[0] == counts[1], "a later block call allocates"


# ------------------------------------------------------------------------------------------------
# 10. round trip with the half solves
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
def test_round_trip_with_the_half_solves(f32, ca, spd):
    name = "lapl_3375x3375"
    S = spd(name)
    dev, arena, _ = device_of(ca, "spd:" + name, S.plan, f32)
    dev.set_option("multiply_nrhs_min", BLOCK)
    n, k = S.n, 33
    tol = S.tol_forward(U32 if f32 else U64)
    Wn = np.random.default_rng(50).standard_normal((n, k))
    for which, Z in ((FWD, Wn), (BWD, Wn / S.s[:, None])):   # FORWARD: M z scales like a right-hand side; BACKWARD: z scales like a solution
        Zg, Yg = block(Z), empty_block(n, k)
        dev.multiply_half_nrhs(arena, Zg.t, Yg.t, which)
        dev.solve_half_nrhs(arena, Yg.t, Yg.t, which)
        dev.sync()
        Yg.assert_guards("round trip")
        X = Yg.numpy()
        e = max(float(np.abs(X[:, j] - Z[:, j]).max() / np.abs(Z[:, j]).max()) if which == FWD else S.forward_error(X[:, j], Z[:, j]) for j in range(k))
        print(f"{name} {PIDS[f32]} round trip which={which}: {e:.3e} (tol {tol:.3e}, ratio {e / tol:.3e})")
        assert e <= tol


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    poison_child()
