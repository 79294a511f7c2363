"""Selected inversion on the GPU (cholamd_selinv, cholamd_selinv_diag, cholamd_selinv_entries, cholamd_mmat --invdiag), all through the C ABI.

Reference, mask, measure and bound are selinv_ref's (see its docstring): Zref = inv(P A P^T) dense with two long-double refinement steps; the mask
is L_oracle != 0 plus tril(P A P^T); every masked entry is gated at C_SEL (k + 1) u r_i r_j in the equilibrated matrix, C_SEL = 8, and a masked
entry that is not finite fails.  The diagonal and the entries in original order are gated by the same bound for their own (i, j).  Every test
prints the largest observed ratio before it asserts (-s)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import selinv_ref as sr  # noqa: E402
import spd_inputs as si  # noqa: E402
from conftest import CASES, ROOT, case_paths  # noqa: E402

BIN = os.path.join(ROOT, "cholesky_amd", "bin", "cholamd_mmat")


@pytest.fixture(scope="module")
def spd(tmp_path_factory):
    return lambda name: si.cached(tmp_path_factory, name)


def _factor(plan, opts=None):
    import cholesky_amd as ca
    dev = ca.Device(plan, 0)
    for k, v in (opts or {}).items():
        dev.set_option(k, v)
    arena = dev.new_arena()
    dev.fill(arena)
    dev.factor(arena)
    dev.sync()
    assert dev.info() == (0, 0)
    return dev, arena


def _orig_bound(S, Zr):
    """(Zref in original order, the bound's r in original order)."""
    p = S.perm
    Zo = np.empty_like(Zr)
    Zo[np.ix_(p, p)] = Zr
    r = np.empty(S.n)
    r[p] = np.abs(Zr * S.sp[:, None] * S.sp[None, :]).sum(axis=1)
    return Zo, r


def _check_all(S, dev, zarena, name, Zr=None, diag=None, vals=None):
    """The Z arena on the mask, selinv_diag and selinv_entries against Zref; returns (Zref, the largest ratios)."""
    plan = S.plan
    Zr = sr.zref(S.PAP, S.Ld) if Zr is None else Zr
    mask = sr.mask_of(S)
    za = zarena.cpu().numpy() if hasattr(zarena, "cpu") else zarena
    Z = plan.arena_to_dense(za)
    q, left_out = sr.ratio(S, Z, Zr, mask)
    Zo, r = _orig_bound(S, Zr)
    unit = (S.k + 1) * si.U64
    d = (dev.selinv_diag(zarena) if diag is None else diag).cpu().numpy()
    dev.sync()
    assert np.array_equal(d[S.perm], np.diag(Z))                        # the walk of factor_diag over the Z arena
    qd = float(np.max(np.where(np.isfinite(d), np.abs(d - np.diag(Zo)) * S.s * S.s / (unit * r * r), np.inf)))
    v = (dev.selinv_entries(zarena) if vals is None else vals).cpu().numpy()
    row, col = plan.entries()
    inpat = np.zeros(plan.nz, dtype=bool)
    inpat[plan.value_map()] = True
    assert np.isnan(v[~inpat]).all() and np.isfinite(v[inpat]).all()
    i, j = row[inpat], col[inpat]
    qe = float(np.max(np.abs(v[inpat] - Zo[i, j]) * S.s[i] * S.s[j] / (unit * r[i] * r[j])))
    print(f"selinv gpu {name}: n = {S.n}, k = {S.k}, mask = {int(mask.sum())}, max ratio arena / diag / entries = {q:.3g} / {qd:.3g} / {qe:.3g} (bound {sr.C_SEL})")
    assert left_out == 0
    assert q <= sr.C_SEL and qd <= sr.C_SEL and qe <= sr.C_SEL, (name, q, qd, qe)
    return Zr, (q, qd, qe)


@pytest.mark.parametrize("case", list(CASES))
def test_fixtures(case):
    """The reference's four fixtures with their own values; the factor comes from the one-launch program."""
    S = sr.Fixture(case)
    dev, arena = _factor(S.plan)
    z = dev.selinv(arena)
    dev.sync()
    _check_all(S, dev, z, case)


@pytest.mark.parametrize("name", si.NAMES)
def test_general_spd_inputs(name, spd):
    S = spd(name)
    dev, arena = _factor(S.plan)
    z = dev.selinv(arena)
    dev.sync()
    _check_all(S, dev, z, name)


def test_generated_grid_with_split_pivots_and_determinism(tmp_path):
    """20^3 (n = 8000, root separator of 400 columns = 7 column blocks); the factor comes from the level schedule (option "program" = 0; the root's
    400 columns are beyond the program launch anyway) with its pivots split into column blocks (400 > split_min = 144).  The dense reference costs one 8000^3 / 3
    Cholesky, 3 x 2 x 8000^3 flops of triangular solves for the inverse and its two refinements, and five dense 512 MB matrices on the CPU."""
    import torch
    S = si.SPD(str(tmp_path), (20, 20, 20, 4, 32), 77, pattern="own", name="g20")
    root = int(S.plan.tree[0])
    assert S.plan.sep_sizes[root - 1] == 400 and S.plan.selinv_blocks(root) == 7
    dev, arena = _factor(S.plan, {"program": 0})
    z1 = dev.selinv(arena)
    z2 = torch.full_like(z1, float("nan"))
    dev.selinv(arena, z2)
    dev.sync()
    assert torch.equal(z1, z2)                                         # bit for bit, the whole arena (no NaN anywhere: every element is written)
    _check_all(S, dev, z1, "g20 own pattern")


def test_determinism_on_the_fixture():
    import torch
    S = sr.Fixture("lapl_3375x3375")
    dev, arena = _factor(S.plan)
    z = [dev.selinv(arena, torch.full((S.plan.arena_doubles,), float(i), dtype=torch.float64, device="cuda")) for i in range(2)]
    dev.sync()
    assert torch.equal(z[0], z[1]) and bool(torch.isfinite(z[0]).all())


def test_inverse_follows_set_values(spd, tmp_path):
    """New values on the same plan: the inverse is that of the current values, not of the plan's."""
    S = spd("g12_full")
    S2 = si.SPD(str(tmp_path), (12, 12, 12, 4, 16), 4242, pattern="full", name="g12_other")
    assert np.array_equal(S2.perm, S.perm)
    row, col = S.plan.entries()
    vals = np.ascontiguousarray(S2.A[row, col])
    dev, arena = _factor(S.plan)
    dev.set_values(vals)
    dev.fill(arena)
    dev.factor(arena)
    dev.sync()
    assert dev.info() == (0, 0)
    z = dev.selinv(arena)
    dev.sync()
    S2.plan = S.plan                                                   # the layout is S's; the references are S2's
    _check_all(S2, dev, z, "g12_full after set_values")


def test_entries_outside_the_pattern_are_nan(tmp_path):
    """An explicit zero in the matrix file is an entry of the value array without a position in any arena: NaN, the others as usual."""
    import cholesky_amd as ca
    S = si.SPD(str(tmp_path), (7, 5, 3, 3, 4), 11, pattern="subset", p=0.5, name="sub")
    free = np.argwhere(np.tril(S.A == 0, -1))
    i, j = (int(v) for v in free[len(free) // 2])
    row, col, val = np.append(S.row, i), np.append(S.col, j), np.append(S.val, 0.0)
    S.mtx = os.path.join(str(tmp_path), "sub_zero.mtx")
    si.write_mtx(S.mtx, S.n, row, col, val)
    S.plan = ca.Plan(S.mtx, S.ord, S.clust)
    assert S.plan.nz == len(val) and S.plan.nnz_a == len(val) - 1 and np.array_equal(S.plan.perm, S.perm)
    dev, arena = _factor(S.plan)
    z = dev.selinv(arena)
    v = dev.selinv_entries(z).cpu().numpy()
    r, c = S.plan.entries()
    k = int(np.nonzero((r == i) & (c == j))[0][0])
    assert np.isnan(v[k]) and np.isnan(v).sum() == 1
    _check_all(S, dev, z, "subset with an explicit zero")


def test_diag_equals_norms_of_half_solves():
    """(A^-1)_ii = ||M^-1 e_i||^2: selinv_diag against the column sums of squares of solve_half_nrhs(FORWARD) of the identity on lapl_400x400.  Both
    sides carry the bound's error, so the gate is twice it."""
    import torch
    S = sr.Fixture("lapl_400x400")
    n = S.n
    dev, arena = _factor(S.plan)
    z = dev.selinv(arena)
    d = dev.selinv_diag(z).cpu().numpy()
    B = torch.eye(n, dtype=torch.float64, device="cuda").T
    X = torch.empty(n, n, dtype=torch.float64, device="cuda").T
    dev.solve_half_nrhs(arena, B, X, dev.HALF_FORWARD)
    dev.sync()
    h = (X.cpu().numpy() ** 2).sum(axis=0)
    Zr = sr.zref(S.PAP, S.Ld)
    _, r = _orig_bound(S, Zr)
    q = float(np.max(np.abs(d - h) * S.s * S.s / ((S.k + 1) * si.U64 * r * r)))
    print(f"selinv diag vs half solves: max ratio = {q:.3g} (bound {2 * sr.C_SEL})")
    assert q <= 2 * sr.C_SEL


def test_argument_errors():
    import ctypes as C
    import torch
    import cholesky_amd as ca
    S = sr.Fixture("lapl_400x400")
    plan = S.plan
    dev, arena = _factor(plan)
    na, L = plan.arena_doubles, dev.L
    big = torch.full((na + 16,), 7.0, dtype=torch.float64, device="cuda")
    big[:na].copy_(arena)
    with pytest.raises(ca.CholamdError, match="overlaps"):
        dev.selinv(arena, arena)
    with pytest.raises(ca.CholamdError, match="overlaps"):
        dev.selinv(big[:na], big[16:])
    dev.sync()
    assert torch.equal(big[:na], arena) and bool((big[na:] == 7.0).all())     # nothing written
    z = dev.selinv(arena)
    p = C.c_void_p(z.data_ptr())
    assert L.cholamd_selinv(dev.h, None, p, None) == -4 and L.cholamd_selinv(dev.h, p, None, None) == -4
    assert L.cholamd_selinv_diag(dev.h, None, p, None) == -4 and L.cholamd_selinv_diag(dev.h, p, None, None) == -4
    assert L.cholamd_selinv_entries(dev.h, None, p, plan.nz, None) == -4 and L.cholamd_selinv_entries(dev.h, p, None, plan.nz, None) == -4
    out = torch.full((plan.nz + 1,), 3.0, dtype=torch.float64, device="cuda")
    for count in (plan.nz - 1, plan.nz + 1, 0):
        assert L.cholamd_selinv_entries(dev.h, p, C.c_void_p(out.data_ptr()), count, None) == -4
    dev.sync()
    assert bool((out == 3.0).all())
    with pytest.raises(ValueError):
        dev.selinv_diag(z, out=torch.empty(plan.n + 1, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        dev.selinv_entries(z, out=torch.empty(plan.nz, dtype=torch.float32, device="cuda"))


def test_failed_factorisation_returns(spd):
    """A pivot that fails (A'_kk = A_kk - 1.5 L_kk^2 in the middle of the matrix, test_gpu_general_spd's construction): the call returns, the numbers
    mean nothing, the pivot is still reported."""
    import torch
    import cholesky_amd as ca
    S = spd("g12_full")
    P = S.plan
    k = S.n // 2
    host = P.fill_host()
    lbl, off = S.sep_of(k)
    b = P.blocks[(P.blocks[:, 0] == lbl) & (P.blocks[:, 1] == lbl)][0]
    j = k - off
    idx = int(b[7]) + j + j * int(b[6])
    assert host[idx] == S.PAP[k, k]
    host[idx] = S.PAP[k, k] - 1.5 * S.Ld[k, k] ** 2
    dev = ca.Device(P, 0)
    bad = torch.from_numpy(host).cuda()
    dev.factor(bad)
    dev.sync()
    info = dev.info()
    assert info[0] > 0
    z = dev.selinv(bad)
    dev.selinv_diag(z)
    dev.selinv_entries(z)
    dev.sync()
    assert dev.info() == info


def poison_child():
    """Runs in a child process with CHOLAMD_POISON=1: guarded, NaN-filled caller buffers."""
    from guarded import Guarded
    assert os.environ.get("CHOLAMD_POISON") == "1"
    S = sr.Fixture("lapl_3375x3375")
    plan = S.plan
    dev, _ = _factor(plan)
    a = Guarded(plan.arena_doubles)
    dev.fill(a.t)
    dev.factor(a.t)
    dev.sync()
    assert dev.info() == (0, 0)
    snap = a.snapshot()
    z, d, v = Guarded(plan.arena_doubles), Guarded(plan.n), Guarded(plan.nz)
    assert np.isnan(z.numpy()).all() and np.isnan(d.numpy()).all() and np.isnan(v.numpy()).all()
    dev.selinv(a.t, z.t)
    dev.selinv_diag(z.t, out=d.t)
    dev.selinv_entries(z.t, out=v.t)
    dev.sync()
    a.assert_unchanged(snap, "arena")
    for g, what in ((z, "Z arena"), (d, "diag"), (v, "entries")):
        g.assert_guards(what)
    assert np.isfinite(z.numpy()).all()
    _check_all(S, dev, z.numpy(), "lapl_3375x3375 poisoned", diag=d.t, vals=v.t)
    print("poison child ok")


def test_poisoned_scratch_and_guarded_buffers():
    env = dict(os.environ, CHOLAMD_POISON="1")
    code = f"import sys; sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); import conftest, test_gpu_selinv as t; t.poison_child()"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0 and "poison child ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("full", [False, True])
def test_cli_invdiag(full, tmp_path):
    case = "lapl_3375x3375"
    m, o, c, _ = case_paths(case)
    out = tmp_path / "invdiag.txt"
    r = subprocess.run([BIN, "-i", m, "-s", o, "-c", c, "--invdiag", str(out)] + (["--full-precision"] if full else []), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Saving diagonal of the inverse to:" in r.stdout
    d = np.genfromtxt(str(out)).reshape(-1)
    S = sr.Fixture(case)
    Zo, rr = _orig_bound(S, sr.zref(S.PAP, S.Ld))
    ref = np.diag(Zo)
    if full:
        q = float(np.max(np.abs(d - ref) * S.s * S.s / ((S.k + 1) * si.U64 * rr * rr)))
        print(f"--invdiag --full-precision: max ratio = {q:.3g}")
        assert q <= sr.C_SEL
    else:
        assert len(d) == S.n and np.abs(d / ref - 1.0).max() <= 5.1e-8           # %0.8g: eight significant digits
