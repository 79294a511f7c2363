"""The factor applied forwards on the device: y = M z, M^T z, M M^T z and the factor residual (cholamd_multiply_half*, cholamd_multiply*,
cholamd_factor_residual*), M = P^T L P in original dof order.

Gates -- none is measured from the code under test; u = 2^-53 in the products (their arithmetic is fp64 for either factor), and u = U64 / U32 where the
factor's own error enters.
 1. Against the device's own factor (downloaded, tril of its image, an fp32 factor converted to fp64): componentwise (k + 2) u |L| |z|, the
    inner-product bound of multiply_ref, k = the most non-zero terms of a component.
 2. Against an independent factor Lr (the CPU oracle's on the fixtures, the dense fp64 Cholesky factor of P A P^T on spd_inputs.NAMES): two factors of
    one matrix differ per entry by |L - Lr|_ij <= tol_factor(u) sqrt(A_ii) (spd_inputs: C_L (k + 1) u kappa, row-scaled), and |Lr_ij| <= sqrt(A_ii), so
      FORWARD   |y - yr|_i <= (tol_factor(u) + (k + 2) U64) sqrt(A_ii) sum_{j in row i} |z_j|
      BACKWARD  |y - yr|_j <= (tol_factor(u) + (k + 2) U64) sum_{i in column j} sqrt(A_ii) |z_i|
    over the pattern of Lr, the second term being gate 1 of the product itself.
 3. Round trip solve_half(w)(multiply_half(w)(z)) against z: the product is backward stable (gate 1), the half solve's forward error is
    tol_forward(u) = C_FE (k + 1) u kappa in the measures of test_gpu_factor_query (FORWARD: max-norm relative, BACKWARD: SPD.forward_error).
 4. multiply against A z: M M^T = A + dA with |dA| <= gamma_(k+1) |L| |L^T| (Higham Thm 10.3) and each of the two products adds (k + 2) u |L| |L^T| |z|
    at most: |y - A z| <= C_BE (k + 1) u |L| |L^T| |z| componentwise, C_BE = 4 >= 3.
10. factor_residual: the 2-norm of the same componentwise bound, || C_BE (k + 1) u |Lr| |Lr^T| |z| ||_2 / ||A z||_2 with the REFERENCE factor Lr (first order:
    |L| |L^T| and |Lr| |Lr^T| differ by O(u)); it is at most C_BE (k + 1) u kappa sqrt(n) ||s||_2 / s_min for a probe z = S^-1 w, and far tighter.

There is no block (nrhs) form in this version.  The size constants of the new kernels are the 16-line tile of an item (CHOL_MUL_TILE) and the 256
reduction steps per staged block of z (MUL_THREADS).

Every test prints its largest error / gate ratio with pytest -s; DESIGN.md section 13 records them once they have been taken on an MI355X."""
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
from oracle import oracle as orc  # noqa: E402
from spd_inputs import C_BE, C_L, U32, U64  # noqa: E402

FWD, BWD = 0, 1
PRECISIONS = [False, True]
PIDS = ["fp64", "fp32"]
GENERATED = {"gen_12x12x12": (12, 12, 12, 4, 16)}
TREE_NAMES = tree_inputs.NAMED + tree_inputs.SINGLE
# separator sizes one below, at and one above every size constant of the new kernels
SWEEP = [15, 16, 17,        # CHOL_MUL_TILE = 16: the lines of an item, the last item of a separator
         255, 256, 257]     # MUL_THREADS = 256: reduction steps per staged block of z
POISON_INPUTS = ["lapl_400x400", "tree_over"]


@pytest.fixture(scope="module")
def ca():
    import cholesky_amd
    orc.use_own_kernels()
    return cholesky_amd


@pytest.fixture(scope="module")
def spd(tmp_path_factory):
    return lambda name: tree_inputs.cached(tmp_path_factory, name)


def cuda(v):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).cuda()


def nan_vec(n):
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def factored(ca, plan, f32):
    dev = ca.Device(plan, 0)
    a = dev.new_arena_f32() if f32 else dev.new_arena()
    (dev.fill_f32 if f32 else dev.fill)(a)
    (dev.factor_f32 if f32 else dev.factor)(a)
    dev.sync()
    assert dev.info() == (0, 0)
    return dev, a


_DEV = {}


def device_of(ca, key, plan, f32):
    """(dev, arena, tril of the arena's image as CSR) of a factored plan, cached."""
    if (key, f32) not in _DEV:
        dev, a = factored(ca, plan, f32)
        _DEV[key, f32] = (dev, a, si.arena_to_sparse(plan, a.cpu().numpy().astype(np.float64)))
    return _DEV[key, f32]


def half(dev, arena, z, which):
    y = nan_vec(len(z))
    dev.multiply_half(arena, cuda(z), y, which)
    dev.sync()
    return y.cpu().numpy()


def full(dev, arena, z):
    y = nan_vec(len(z))
    dev.multiply(arena, cuda(z), y)
    dev.sync()
    return y.cpu().numpy()


def own_factor_ratio(dev, arena, Dsp, perm, z, tag):
    """Gate 1 for both halves, out of place (y prefilled with NaN) and in place; the largest error / gate ratio."""
    worst = 0.0
    for which in (FWD, BWD):
        yref, absprod, k = mr.product_sparse(Dsp, perm, z, which)
        y = half(dev, arena, z, which)
        r = mr.gate_ratio(y, yref, absprod, k)
        print(f"{tag} which={which}: error / gate = {r:.3f} (k = {k})")
        assert r <= 1.0, (tag, which, r)
        t = cuda(z)
        dev.multiply_half(arena, t, t, which)
        dev.sync()
        assert np.array_equal(t.cpu().numpy(), y), "in place: the same bits"
        worst = max(worst, r)
    return worst


def plain_plan(ca, name):
    if name in CASES:
        return ca.Plan(*case_paths(name)[:3])
    g = GENERATED[name]
    return ca.Problem(*g[:3], levels=g[3], tile=g[4]).plan()


# ------------------------------------------------------------------------------------------------
# 1. against the device's own factor
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("name", list(CASES) + list(GENERATED))
def test_products_match_the_downloaded_factor(name, f32, ca):
    plan = plain_plan(ca, name)
    dev, arena, Dsp = device_of(ca, name, plan, f32)
    z = np.random.default_rng(21).standard_normal(plan.n)
    own_factor_ratio(dev, arena, Dsp, plan.perm, z, f"{name} {PIDS[f32]}")


# ------------------------------------------------------------------------------------------------
# 2. against an independent factor
# ------------------------------------------------------------------------------------------------
def independent_ratio(dev, arena, Lr, perm, sp, tolf, z, tag):
    import scipy.sparse as sps
    Lsp = sps.csr_matrix(np.tril(Lr))
    pat = Lsp.copy()
    pat.data[:] = 1.0
    worst = 0.0
    for which in (FWD, BWD):
        yref, _, k = mr.product_sparse(Lsp, perm, z, which)
        zp = np.abs(z[perm])
        b = np.empty(len(z))
        b[perm] = (tolf + (k + 2) * U64) * (sp * (pat @ zp) if which == FWD else pat.T @ (sp * zp))
        y = half(dev, arena, z, which)
        assert np.isfinite(y).all()
        r = float((np.abs(y - yref) / b).max())
        print(f"{tag} which={which}: error / gate = {r:.3e}")
        assert r <= 1.0, (tag, which, r)
        worst = max(worst, r)
    return worst


@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("case", list(CASES))
def test_products_on_fixtures_match_the_oracle(case, f32, ca, golden):
    m, o, c, _ = case_paths(case)
    plan = ca.Plan(m, o, c)
    O = orc.Oracle(m, o, c)
    O.factor()
    assert O.info == 0 and np.array_equal(np.asarray(O.perm), plan.perm)
    g = golden(case)
    PAP = g["pmat"] + np.tril(g["pmat"], -1).T
    sp = np.sqrt(np.diag(PAP))
    ev = np.linalg.eigvalsh(PAP / sp[:, None] / sp[None, :])
    Lo = np.tril(O.dense())
    k = int((g["L"] != 0).sum(axis=1).max())
    tolf = C_L * (k + 1) * (U32 if f32 else U64) * float(ev[-1] / ev[0])
    dev, arena, _ = device_of(ca, case, plan, f32)
    z = np.random.default_rng(22).standard_normal(plan.n)
    independent_ratio(dev, arena, Lo, plan.perm, sp, tolf, z, f"{case} {PIDS[f32]} oracle")


@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("name", si.NAMES)
def test_products_on_general_inputs_match_the_dense_factor(name, f32, ca, spd):
    S = spd(name)            # no input is excluded for the fp32 factor
    dev, arena, _ = device_of(ca, "spd:" + name, S.plan, f32)
    z = np.random.default_rng(23).standard_normal(S.n)
    independent_ratio(dev, arena, S.Ld, S.perm, S.sp, S.tol_factor(U32 if f32 else U64), z, f"{name} {PIDS[f32]} dense")


# ------------------------------------------------------------------------------------------------
# 3. round trip, 4. multiply against A z
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("name", si.NAMES)
def test_round_trip_and_full_product(name, f32, ca, spd):
    S = spd(name)
    dev, arena, Dsp = device_of(ca, "spd:" + name, S.plan, f32)
    u = U32 if f32 else U64
    tol = S.tol_forward(u)
    w = np.random.default_rng(24).standard_normal(S.n)
    for which, z in ((FWD, w), (BWD, w / S.s)):   # FORWARD: M z scales like a right-hand side; BACKWARD: z scales like a solution
        t = cuda(z)
        y = nan_vec(S.n)
        dev.multiply_half(arena, t, y, which)
        dev.solve_half(arena, y, y, which)
        dev.sync()
        x = y.cpu().numpy()
        e = float(np.abs(x - z).max() / np.abs(z).max()) if which == FWD else S.forward_error(x, z)
        print(f"{name} {PIDS[f32]} round trip which={which}: {e:.3e} (tol {tol:.3e}, ratio {e / tol:.3e})")
        assert e <= tol
    z = w / S.s
    y = full(dev, arena, z)
    az = S.A_sparse @ z
    aD = abs(Dsp)
    bound = np.empty(S.n)
    bound[S.perm] = C_BE * (S.k + 1) * u * (aD @ (aD.T @ np.abs(z[S.perm])))
    assert np.isfinite(y).all()
    r = float((np.abs(y - az) / bound).max())
    print(f"{name} {PIDS[f32]} M M^T z against A z: error / gate = {r:.3e}")
    assert r <= 1.0
    t = cuda(z)
    dev.multiply(arena, t, t)
    dev.sync()
    assert np.array_equal(t.cpu().numpy(), y), "in place: the same bits"


# ------------------------------------------------------------------------------------------------
# 6. determinism
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("name", ["lapl_3375x3375", "tree_over"])
def test_two_calls_return_the_same_bits(name, f32, ca, spd):
    import torch
    plan = plain_plan(ca, name) if name in CASES else spd(name).plan
    dev, arena, _ = device_of(ca, name if name in CASES else "spd:" + name, plan, f32)
    n = plan.n
    z = cuda(np.random.default_rng(26).standard_normal(n))
    outs = []
    for _ in range(2):
        o = []
        for which in (FWD, BWD):
            y = nan_vec(n)
            dev.multiply_half(arena, z, y, which)
            o.append(y)
        y = nan_vec(n)
        dev.multiply(arena, z, y)
        o.append(y)
        dev.sync()
        outs.append(o)
    for a, b in zip(*outs):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    r1, r2 = dev.factor_residual(arena, z), dev.factor_residual(arena, z)
    assert r1 == r2 and np.isfinite(r1)


# ------------------------------------------------------------------------------------------------
# 7. trees
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TREE_NAMES)
def test_products_on_trees(name, ca, spd):
    S = spd(name)
    z = np.random.default_rng(27).standard_normal(S.n)
    for f32 in PRECISIONS:
        dev, arena, Dsp = device_of(ca, "spd:" + name, S.plan, f32)
        own_factor_ratio(dev, arena, Dsp, S.perm, z, f"{name} {PIDS[f32]}")


@pytest.mark.parametrize("s", SWEEP)
@pytest.mark.parametrize("position", ["leaf", "middle", "root"])
def test_products_at_kernel_size_constants(position, s, ca, tmp_path):
    S = tree_inputs.sweep(tmp_path, position, s, leaf=("band", 20) if position == "leaf" and s > 32 else "dense", oracle=False)
    z = np.random.default_rng(28).standard_normal(S.n)
    for f32 in PRECISIONS:
        dev, a = factored(ca, S.plan, f32)
        Dsp = si.arena_to_sparse(S.plan, a.cpu().numpy().astype(np.float64))
        own_factor_ratio(dev, a, Dsp, S.perm, z, f"sweep {position} {s} {PIDS[f32]}")


# ------------------------------------------------------------------------------------------------
# 8. poison: a fresh child process per setting, the same uploaded arena, the same bits
# ------------------------------------------------------------------------------------------------
def poison_child():
    """Both halves and the full product of POISON_INPUTS on an arena uploaded from the host (the dense factor on the lower triangle, NaN elsewhere),
    printed as hex words: the parent compares the output of a poisoned and an unpoisoned child."""
    import cholesky_amd as ca
    import torch
    with tempfile.TemporaryDirectory() as tmp:
        for name in POISON_INPUTS:
            if name in CASES:
                plan = ca.Plan(*case_paths(name)[:3])
            else:
                spec = tree_inputs.TREES[name]
                plan = si.SPD(tmp, spec, 3000 + spec["seed"], name=name, oracle=False, dense=False).plan
            D = plan.arena_to_dense(plan.fill_host())
            host = mr.arena_from_lower(plan, np.linalg.cholesky(np.tril(D) + np.tril(D, -1).T))
            z = np.random.default_rng(29).standard_normal(plan.n)
            for f32 in PRECISIONS:
                dev = ca.Device(plan, 0)
                arena = torch.from_numpy(host.astype(np.float32) if f32 else host).cuda()
                outs = [half(dev, arena, z, FWD), half(dev, arena, z, BWD), full(dev, arena, z)]
                for tag, v in zip(("forward", "backward", "full"), outs):
                    assert np.isfinite(v).all(), (name, f32, tag)
                    print(name, PIDS[f32], tag, v.view(np.uint64).tobytes().hex())
    print("poison child: ok")


def test_poisoned_buffers_change_nothing():
    outs = []
    for poison in ("0", "1"):
        env = dict(os.environ, CHOLAMD_POISON=poison)
        for v in ("CHOLAMD_SOLVE_NO_BAND", "CHOLAMD_COMPACT"):
            env.pop(v, None)
        p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and "poison child: ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
        outs.append(p.stdout)
    assert outs[0].count("\n") == 3 * 2 * len(POISON_INPUTS) + 1
    assert outs[0] == outs[1], "the poisoned run returns other bits"


# ------------------------------------------------------------------------------------------------
# 9. arguments
# ------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_untouched(ca):
    import ctypes as C
    import math
    import torch
    plan = plain_plan(ca, "lapl_400x400")
    n = plan.n
    V = np.random.default_rng(30).standard_normal((n, 1))
    msg = lambda: ca.load().cholamd_last_error().decode()  # noqa: E731
    for f32 in PRECISIONS:
        dev, arena, _ = device_of(ca, "lapl_400x400", plan, f32)
        L, h, p = dev.L, dev.h, dev.ptr
        sfx = "_f32" if f32 else ""
        one, mul, res = getattr(L, "cholamd_multiply_half" + sfx), getattr(L, "cholamd_multiply" + sfx), getattr(L, "cholamd_factor_residual" + sfx)
        z, y = cuda(V[:, 0]), nan_vec(n)
        assert one(h, p(arena), p(z), p(y), 2, None) == -4 and "which" in msg()
        assert one(h, p(arena), p(z), p(y), -1, None) == -4
        assert one(h, p(arena), None, p(y), FWD, None) == -4 and "NULL" in msg()
        assert one(h, None, p(z), p(y), FWD, None) == -4
        assert one(h, p(arena), p(z), None, BWD, None) == -4
        assert one(None, p(arena), p(z), p(y), BWD, None) == -4
        assert mul(h, p(arena), None, p(y), None) == -4 and mul(h, None, p(z), p(y), None) == -4 and mul(h, p(arena), p(z), None, None) == -4
        # a result inside the arena
        before = arena.clone()
        assert one(h, p(arena), p(z), p(arena), FWD, None) == -4 and "overlaps" in msg()
        assert mul(h, p(arena), p(z), p(arena), None) == -4 and "overlaps" in msg()
        dev.sync()
        assert torch.equal(torch.nan_to_num(arena), torch.nan_to_num(before))
        out = C.c_double(1.0)
        assert res(h, None, p(z), C.byref(out), None) == -4 and math.isnan(out.value)
        out = C.c_double(1.0)
        assert res(h, p(arena), None, C.byref(out), None) == -4 and math.isnan(out.value)
        assert res(h, p(arena), p(z), None, None) == -4
        bad = z.clone()
        bad[7] = float("nan")
        out = C.c_double(1.0)
        assert res(h, p(arena), p(bad), C.byref(out), None) == -4 and math.isnan(out.value) and "finite" in msg()
        with pytest.raises(ca.CholamdError, match="which"):
            dev.multiply_half(arena, z, y, 2)
        with pytest.raises(ValueError):
            dev.multiply_half(arena, z[:-1], y, FWD)
        with pytest.raises(ValueError):
            dev.multiply(arena, z, y.float())
        dev.sync()
        assert torch.isnan(y).all()
        # another rank of a partitioned object holds no complete factor
        part = ca.Device(plan, 0)
        part.set_partition(1, 2)
        assert one(part.h, p(arena), p(z), p(y), FWD, None) == -4 and "complete factor" in msg()
        assert mul(part.h, p(arena), p(z), p(y), None) == -4
        out = C.c_double(1.0)
        assert res(part.h, p(arena), p(z), C.byref(out), None) == -4 and math.isnan(out.value)
        part.sync()
        assert torch.isnan(y).all()


# ------------------------------------------------------------------------------------------------
# 10. factor_residual
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lapl_3375x3375", "lapl_3375_scaled"])
def test_factor_residual(name, ca, spd):
    S = spd(name)
    z = np.random.default_rng(31).standard_normal(S.n) / S.s
    aL = np.abs(np.tril(S.Ld))
    amp = np.linalg.norm(aL @ (aL.T @ np.abs(z[S.perm]))) / np.linalg.norm(S.A_sparse @ z)

    def bound(u):
        return C_BE * (S.k + 1) * u * amp

    vals = np.ascontiguousarray(S.val[np.lexsort((S.row, S.col))])
    rel = {}
    for f32 in PRECISIONS:
        dev, arena = factored(ca, S.plan, f32)        # (its own device object: the values change below)
        d_z = cuda(z)
        rel[f32] = dev.factor_residual(arena, d_z)
        b = bound(U32 if f32 else U64)
        print(f"{name} {PIDS[f32]}: factor residual {rel[f32]:.3e} (bound {b:.3e}, ratio {rel[f32] / b:.3e})")
        assert rel[f32] <= b
        dev.set_values(1.5 * vals)                    # the arena still factors the old values: |A' z - A z| / |A' z| = 1/3
        stale = dev.factor_residual(arena, d_z)
        print(f"{name} {PIDS[f32]}: after set_values(1.5 A) without a factorisation {stale:.6f}")
        assert stale >= 0.3
        (dev.fill_f32 if f32 else dev.fill)(arena)
        (dev.factor_f32 if f32 else dev.factor)(arena)
        dev.sync()
        assert dev.info() == (0, 0)
        again = dev.factor_residual(arena, d_z)
        print(f"{name} {PIDS[f32]}: refactored {again:.3e}")
        assert again <= b
    assert rel[True] > rel[False]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    poison_child()
