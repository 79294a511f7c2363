"""Schur complement on the top of the tree on the GPU (cholamd_schur_factor, cholamd_schur, cholamd_schur_condense / _expand and their _f32 forms,
cholamd_mmat --schur), all through the C ABI.

Reference: numpy on the plan's own dense image of the filled arena, A = tril(D) + tril(D, -1)^T, I = [0, t0), T = [t0, n):
S_ref = A_TT - A_TI solve(A_II, A_IT), g_ref = b_T - A_TI solve(A_II, b_I) (b permuted).  S is gated at 1e-12 max|S_ref|, the project's gate for factor
entries; for the general SPD inputs the gate is max(1e-12, 100 x the relative difference of two CPU routes to S_ref).  Every test prints what it measured
before it asserts (-s).  The references are computed once per (input, k) and shared."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import spd_inputs as si  # noqa: E402
from conftest import CASES, ROOT, case_paths  # noqa: E402

BIN = os.path.join(ROOT, "cholesky_amd", "bin", "cholamd_mmat")
GEN12 = "gen_12x12x12"
# (input, k): m = 3 (one block smaller than a tile); m = 9, five kept blocks; m = 65, 17 kept blocks, tiles without storage; root 225 = 14 * 16 + 1 and
# the per-level path on a problem whose cholamd_factor is the program launch; m = 397, separators of 144, 72, 60, 36, 30, 30, 25
SHAPES = [("lapl_9x9", 1), ("lapl_25x25", 2), ("lapl_400x400", 3), ("lapl_3375x3375", 1), ("lapl_3375x3375", 2), (GEN12, 3)]
IDS = [f"{c}-k{k}" for c, k in SHAPES]
_PLANS, _REFS = {}, {}


def get_plan(case):
    """(plan, b in original order)."""
    import cholesky_amd as ca
    if case not in _PLANS:
        if case == GEN12:
            prob = ca.Problem(12, 12, 12, levels=4, tile=16)
            _PLANS[case] = (prob.plan(), np.asarray(prob.rhs(), dtype=np.float64))
        else:
            m, o, c, b = case_paths(case)
            plan = ca.Plan(m, o, c)
            _PLANS[case] = (plan, np.asarray(ca.plan.read_vector(b, plan.n), dtype=np.float64))
    return _PLANS[case]


def schur_refs(A, b_perm, t0):
    """(S_ref, g_ref) from the permuted dense A and the permuted right-hand side: one LU of A_II serves both."""
    AII, AIT, ATT = A[:t0, :t0], A[:t0, t0:], A[t0:, t0:]
    sol = np.linalg.solve(AII, np.column_stack([AIT, b_perm[:t0]]))
    return ATT - AIT.T @ sol[:, :-1], b_perm[t0:] - AIT.T @ sol[:, -1]


def refs(case, k):
    if (case, k) not in _REFS:
        plan, b = get_plan(case)
        D = plan.arena_to_dense(plan.fill_host())
        A = np.tril(D) + np.tril(D, -1).T
        m = plan.schur_size(k)
        S_ref, g_ref = schur_refs(A, b[plan.perm], plan.n - m)
        _REFS[(case, k)] = {"S": S_ref, "g": g_ref, "m": m, "t0": plan.n - m}
    return _REFS[(case, k)]


def partial(plan, k, timing=False):
    """A device object and an arena eliminated down to level k."""
    import cholesky_amd as ca
    dev = ca.Device(plan, 0)
    arena = dev.new_arena()
    dev.fill(arena)
    if timing:
        dev.set_timing(True)
    dev.schur_factor(arena, k)
    dev.sync()
    assert dev.info() == (0, 0)
    return dev, arena


def structural_zeros(plan, k):
    """The positions of S no record of the gather covers (both triangles), and those between kept separators that are not ancestor and descendant."""
    m = plan.schur_size(k)
    t0 = plan.n - m
    covered = np.zeros((m, m), dtype=bool)
    for off, ld, rows, cols, row0, col0, diag in plan.schur_list(k):
        covered[row0:row0 + rows, col0:col0 + cols] = True
    covered |= covered.T
    unrelated = np.zeros((m, m), dtype=bool)
    offs, sizes = plan.sep_offsets, plan.sep_sizes
    nk = (1 << k) - 1
    for ha in range(1, nk + 1):
        for hb in range(1, nk + 1):
            x, y = max(ha, hb), min(ha, hb)
            while x > y:
                x //= 2
            if x != y:  # neither is an ancestor of the other
                a, b = int(plan.tree[ha - 1]), int(plan.tree[hb - 1])
                unrelated[offs[a - 1] - t0:offs[a - 1] - t0 + sizes[a - 1], offs[b - 1] - t0:offs[b - 1] - t0 + sizes[b - 1]] = True
    assert not (unrelated & covered).any()
    return ~covered, unrelated


@pytest.mark.parametrize("case,k", SHAPES, ids=IDS)
def test_schur_against_the_reference(case, k):
    plan, _ = get_plan(case)
    R = refs(case, k)
    big = case == "lapl_3375x3375"
    dev, arena = partial(plan, k, timing=big)
    if big:  # cholamd_factor of this problem is the one-launch program; schur_factor must be the per-level launches
        t = dev.get_timing()
        dev.set_timing(False)
        print(f"schur_factor launches by kind: {t}")
        assert t["other"][1] == 0 and t["potrf"][1] > 0
    S = dev.schur(arena, k)
    dev.sync()
    assert tuple(S.shape) == (R["m"], R["m"]) and S.stride(0) == 1
    S = S.cpu().numpy()
    err, scale = float(np.abs(S - R["S"]).max()), float(np.abs(R["S"]).max())
    print(f"schur {case} k = {k}: m = {R['m']}, max|S - S_ref| = {err:.3g}, max|S_ref| = {scale:.3g}, ratio to the gate = {err / (1e-12 * scale):.3g}")
    assert np.isfinite(S).all()
    assert err <= 1e-12 * scale
    assert np.array_equal(S, S.T)
    uncovered, unrelated = structural_zeros(plan, k)
    assert (S[uncovered] == 0.0).all() and (S[unrelated] == 0.0).all() and not np.signbit(S[uncovered]).any()
    if (case, k) == ("lapl_400x400", 3):
        assert unrelated.any() and (uncovered & ~unrelated).any(), "unrelated separators and tiles without storage are both on this path"
    assert np.array_equal(S, plan.schur_host(k, arena.cpu().numpy()))            # bit for bit


def _largest_k(plan):
    return min(3, plan.levels - 1)


@pytest.fixture(scope="module")
def spd(tmp_path_factory):
    return lambda name: si.cached(tmp_path_factory, name)


@pytest.mark.parametrize("name", si.NAMES)
def test_general_spd_inputs(name, spd):
    Sp = spd(name)
    plan = Sp.plan
    for k in sorted({1, _largest_k(plan)}):
        m = plan.schur_size(k)
        t0 = plan.n - m
        A = Sp.PAP
        # two CPU routes: LU solve of A_II; the Cholesky factor of P A P^T, whose leading block is that of A_II
        S1 = A[t0:, t0:] - A[:t0, t0:].T @ np.linalg.solve(A[:t0, :t0], A[:t0, t0:])
        S2 = A[t0:, t0:] - Sp.Ld[t0:, :t0] @ Sp.Ld[t0:, :t0].T
        scale = float(np.abs(S1).max())
        route = float(np.abs(S1 - S2).max()) / scale
        gate = max(1e-12, 100.0 * route)
        dev, arena = partial(plan, k)
        S = dev.schur(arena, k).cpu().numpy()
        err = max(float(np.abs(S - S1).max()), float(np.abs(S - S2).max())) / scale
        print(f"schur spd {name} k = {k}: m = {m}, routes differ by {route:.3g}, gate {gate:.3g}, error {err:.3g}, ratio {err / gate:.3g}")
        assert np.isfinite(S).all() and err <= gate
        assert np.array_equal(S, S.T)
        assert np.array_equal(S, plan.schur_host(k, arena.cpu().numpy()))


@pytest.mark.parametrize("case,k", [("lapl_400x400", 3), ("lapl_3375x3375", 1), (GEN12, 2)], ids=["lapl_400-k3", "lapl_3375-k1", "gen12-k2"])
def test_completion(case, k):
    """schur_factor(k) then factor_levels(k - 1, 0) is the level-by-level factorisation, bit for bit; chol(S) is the kept diagonal part of that factor."""
    import torch
    plan, _ = get_plan(case)
    dev, arena = partial(plan, k)
    S = dev.schur(arena, k).cpu().numpy()
    dev.factor_levels(arena, k - 1, 0)
    whole = dev.new_arena()
    dev.fill(whole)
    dev.factor_levels(whole, plan.levels - 1, 0)
    dev.sync()
    assert dev.info() == (0, 0)
    assert torch.equal(arena, whole)
    m = plan.schur_size(k)
    Lt = np.tril(plan.arena_to_dense(whole.cpu().numpy()))[plan.n - m:, plan.n - m:]
    err = float(np.abs(np.linalg.cholesky(S) - Lt).max())
    print(f"completion {case} k = {k}: max|chol(S) - L_TT| = {err:.3g}")
    assert err <= 1e-12


@pytest.mark.parametrize("case,k", SHAPES, ids=IDS)
def test_condense_and_expand(case, k):
    import torch
    plan, b = get_plan(case)
    R = refs(case, k)
    dev, arena = partial(plan, k)
    S = dev.schur(arena, k).cpu().numpy()
    d_b = torch.from_numpy(b).cuda()
    w, g = dev.schur_condense(arena, k, d_b)
    dev.sync()
    gh = g.cpu().numpy()
    gerr, gscale = float(np.abs(gh - R["g"]).max()), float(np.abs(R["g"]).max())
    xt = torch.from_numpy(np.linalg.solve(S, gh)).cuda()
    w0 = w.clone()
    x = dev.schur_expand(arena, k, w, xt)
    x2 = dev.schur_expand(arena, k, w, xt)
    dev.sync()
    assert torch.equal(w, w0), "expand must not modify w"
    res = dev.residual(d_b, x)
    dev.factor_levels(arena, k - 1, 0)                      # the completed factor: the plain solve is the yardstick
    xs = torch.empty_like(x)
    dev.solve(arena, d_b, xs)
    dev.sync()
    xh, xsh = x.cpu().numpy(), xs.cpu().numpy()
    rel = float(np.abs(xh - xsh).max() / np.abs(xsh).max())
    again = float(np.abs(x2.cpu().numpy() - xh).max() / np.abs(xh).max())
    print(f"condense/expand {case} k = {k}: |g - g_ref| / max|g_ref| = {gerr / gscale:.3g}, residual = {res:.3g}, x vs solve = {rel:.3g}, second expand = {again:.3g}")
    assert gerr <= 1e-12 * gscale
    assert res <= 1e-10 and rel <= 1e-10
    assert again <= 1e-12                                    # to rounding (the off-diagonal blocks accumulate by atomics): the gate of a factor entry


@pytest.mark.parametrize("case,k", [("lapl_400x400", 3), ("lapl_3375x3375", 1)], ids=["lapl_400-k3", "lapl_3375-k1"])
def test_fp32_arena(case, k):
    """Condense and expand on an fp32 arena eliminated by factor_levels_f32, S from the fp64 run.  The error of x is held against what solve_f32 loses
    against solve on the same case, times 10."""
    import torch
    plan, b = get_plan(case)
    dev, arena = partial(plan, k)
    S = dev.schur(arena, k).cpu().numpy()
    d_b = torch.from_numpy(b).cuda()
    a32 = dev.new_arena_f32()
    dev.fill_f32(a32)
    dev.factor_levels_f32(a32, plan.levels - 1, k)
    dev.sync()
    assert dev.info() == (0, 0)
    w, g = dev.schur_condense(a32, k, d_b)
    dev.sync()
    xt = torch.from_numpy(np.linalg.solve(S, g.cpu().numpy())).cuda()
    x = dev.schur_expand(a32, k, w, xt).cpu().numpy()
    # yardsticks: the fp64 solve and the fp32-factor solve of the same system
    dev.factor_levels(arena, k - 1, 0)
    x64 = torch.empty(plan.n, dtype=torch.float64, device="cuda")
    dev.solve(arena, d_b, x64)
    full32 = dev.new_arena_f32()
    dev.fill_f32(full32)
    dev.factor_f32(full32)
    x32 = torch.empty_like(x64)
    dev.solve_f32(full32, d_b, x32)
    dev.sync()
    x64, x32 = x64.cpu().numpy(), x32.cpu().numpy()
    yard = float(np.abs(x32 - x64).max() / np.abs(x64).max())
    err = float(np.abs(x - x64).max() / np.abs(x64).max())
    print(f"fp32 arena {case} k = {k}: error of x = {err:.3g}, solve_f32 vs solve = {yard:.3g}, ratio = {err / yard:.3g} (bound 10)")
    assert np.isfinite(x).all() and yard > 0 and err <= 10.0 * yard


def test_two_schur_calls_are_bit_identical():
    import torch
    plan, _ = get_plan("lapl_3375x3375")
    k = 2
    dev, arena = partial(plan, k)
    m = plan.schur_size(k)
    outs = [dev.schur(arena, k, out=torch.full((m, m), float(i + 1), dtype=torch.float64, device="cuda").T) for i in range(2)]
    dev.sync()
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all())


def test_argument_errors():
    import ctypes as C
    import torch
    import cholesky_amd as ca
    plan, b = get_plan("lapl_400x400")
    k, n, na, Lv = 2, plan.n, plan.arena_doubles, plan.levels
    dev, arena = partial(plan, k)
    m = plan.schur_size(k)
    L, h = dev.L, dev.h
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    SENT = -7.0
    mk = lambda cnt: torch.full((cnt,), SENT, dtype=torch.float64, device="cuda")  # noqa: E731
    clean = lambda *ts: all(bool((t == SENT).all()) for t in ts)  # noqa: E731
    d_b = torch.from_numpy(b).cuda()
    w_ok, g_ok = dev.schur_condense(arena, k, d_b)
    xt_ok = torch.zeros(m, dtype=torch.float64, device="cuda")
    dev.sync()
    snap = arena.clone()
    Sb, w, g, x = mk(m * (m + 3)), mk(n), mk(m), mk(n)
    # k out of range, everywhere
    for bad in (0, -1, Lv, Lv + 2):
        assert L.cholamd_schur_factor(h, P(arena), bad, None) == -4
        assert L.cholamd_schur(h, P(arena), bad, P(Sb), m, None) == -4
        assert L.cholamd_schur_condense(h, P(arena), bad, P(d_b), P(w), P(g), None) == -4
        assert L.cholamd_schur_expand(h, P(arena), bad, P(w_ok), P(xt_ok), P(x), None) == -4
        assert L.cholamd_schur_condense_f32(h, P(arena), bad, P(d_b), P(w), P(g), None) == -4
        assert L.cholamd_schur_expand_f32(h, P(arena), bad, P(w_ok), P(xt_ok), P(x), None) == -4
        with pytest.raises(ca.CholamdError):
            dev.schur(arena, bad)
    # NULL pointers
    assert L.cholamd_schur_factor(h, None, k, None) == -4 and L.cholamd_schur_factor(None, P(arena), k, None) == -4
    assert L.cholamd_schur(h, None, k, P(Sb), m, None) == -4 and L.cholamd_schur(h, P(arena), k, None, m, None) == -4
    for args in ((None, P(d_b), P(w), P(g)), (P(arena), None, P(w), P(g)), (P(arena), P(d_b), None, P(g)), (P(arena), P(d_b), P(w), None)):
        assert L.cholamd_schur_condense(h, args[0], k, *args[1:], None) == -4
        assert L.cholamd_schur_condense_f32(h, args[0], k, *args[1:], None) == -4
    for args in ((None, P(w_ok), P(xt_ok), P(x)), (P(arena), None, P(xt_ok), P(x)), (P(arena), P(w_ok), None, P(x)), (P(arena), P(w_ok), P(xt_ok), None)):
        assert L.cholamd_schur_expand(h, args[0], k, *args[1:], None) == -4
        assert L.cholamd_schur_expand_f32(h, args[0], k, *args[1:], None) == -4
    # lds < m
    for lds in (m - 1, 0, -3):
        assert L.cholamd_schur(h, P(arena), k, P(Sb), lds, None) == -4
    # S overlapping the arena; the vectors overlapping each other or the arena
    big = torch.full((na + m * m,), SENT, dtype=torch.float64, device="cuda")
    assert L.cholamd_schur(h, P(big[:na]), k, P(big[na - 1:]), m, None) == -4
    assert L.cholamd_schur(h, P(arena), k, P(arena), m, None) == -4
    wg = mk(n + m)
    assert L.cholamd_schur_condense(h, P(arena), k, P(d_b), P(wg[:n]), P(wg[n - 1:]), None) == -4       # w and g
    assert L.cholamd_schur_condense(h, P(arena), k, P(wg[:n]), P(wg[:n]), P(g), None) == -4               # b and w
    assert L.cholamd_schur_condense(h, P(arena), k, P(wg[:n]), P(w), P(wg[1:]), None) == -4               # b and g
    assert L.cholamd_schur_condense(h, P(big[:na]), k, P(d_b), P(big[na - 1:]), P(g), None) == -4         # w and the arena
    assert L.cholamd_schur_expand(h, P(arena), k, P(wg[:n]), P(xt_ok), P(wg[1:]), None) == -4             # x and w
    assert L.cholamd_schur_expand(h, P(arena), k, P(w_ok), P(wg[:m]), P(wg[m - 1:]), None) == -4          # x and xt
    assert L.cholamd_schur_expand(h, P(big[:na]), k, P(w_ok), P(xt_ok), P(big[na - 1:]), None) == -4      # x and the arena
    # a partitioned device object
    part = ca.Device(plan, 0)
    part.set_partition(0, 2)
    assert L.cholamd_schur_factor(part.h, P(arena), k, None) == -4
    assert L.cholamd_schur(part.h, P(arena), k, P(Sb), m, None) == -4
    assert L.cholamd_schur_condense(part.h, P(arena), k, P(d_b), P(w), P(g), None) == -4
    assert L.cholamd_schur_expand(part.h, P(arena), k, P(w_ok), P(xt_ok), P(x), None) == -4
    assert "partitioned" in L.cholamd_last_error().decode()
    dev.sync()
    assert clean(Sb, w, g, x, big, wg) and torch.equal(arena, snap), "a refused call wrote something"
    # the Python layer's own checks
    with pytest.raises(ValueError):
        dev.schur(arena, k, out=torch.empty(m, m, dtype=torch.float32, device="cuda").T)
    with pytest.raises(ValueError):
        dev.schur(arena, k, out=torch.empty(m, m, dtype=torch.float64, device="cuda")[:, : m - 1].T)
    with pytest.raises(ValueError):
        dev.schur(arena, k, out=torch.empty(m + 1, m + 1, dtype=torch.float64, device="cuda")[:m, :m])   # row-major
    with pytest.raises(ValueError):
        dev.schur_condense(arena, k, d_b, w=torch.empty(n + 1, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        dev.schur_expand(arena, k, w_ok, torch.zeros(m + 1, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        dev.schur(dev.new_arena_f32(), k)
    # a good call into a padded output: rows m .. lds - 1 stay as they were
    out = Sb.view(m, m + 3).T
    S = dev.schur(arena, k, out=out)
    dev.sync()
    assert bool((out[m:, :] == SENT).all()) and np.array_equal(S.cpu().numpy(), plan.schur_host(k, arena.cpu().numpy()))


def poison_child():
    """Runs in a child process with CHOLAMD_POISON=1: guarded, NaN-filled caller buffers; the clean run is the CPU gather / the shared reference."""
    import torch
    from guarded import Guarded
    assert os.environ.get("CHOLAMD_POISON") == "1"
    for case, k in (("lapl_400x400", 3), ("lapl_3375x3375", 1)):
        plan, b = get_plan(case)
        R = refs(case, k)
        m, n = R["m"], plan.n
        dev, arena = partial(plan, k)
        snap = arena.clone()
        S, g, w, x = Guarded(m, m, ld=m + 5), Guarded(m), Guarded(n), Guarded(n)
        d_b = torch.from_numpy(b).cuda()
        dev.schur(arena, k, out=S.t)
        dev.schur_condense(arena, k, d_b, w=w.t, g=g.t)
        dev.sync()
        Sh, gh = S.numpy(), g.numpy()
        xt = torch.from_numpy(np.linalg.solve(Sh, gh)).cuda()
        dev.schur_expand(arena, k, w.t, xt, x=x.t)
        dev.sync()
        for q, what in ((S, "S"), (g, "g"), (w, "w"), (x, "x")):
            q.assert_guards(f"{case} {what}")
            assert np.isfinite(q.numpy()).all(), (case, what)
        assert torch.equal(arena, snap)
        assert np.array_equal(Sh, plan.schur_host(k, arena.cpu().numpy()))                 # the clean run, bit for bit
        assert np.abs(Sh - R["S"]).max() <= 1e-12 * np.abs(R["S"]).max()
        assert np.abs(gh - R["g"]).max() <= 1e-12 * np.abs(R["g"]).max()
        res = dev.residual(d_b, x.t)
        print(f"poisoned {case} k = {k}: residual {res:.3g}")
        assert res <= 1e-10
    print("poison child ok")


def test_poisoned_scratch_and_guarded_buffers():
    env = dict(os.environ, CHOLAMD_POISON="1")
    code = f"import sys; sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); import conftest, test_gpu_schur as t; t.poison_child()"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0 and "poison child ok" in r.stdout, r.stdout + r.stderr


def test_failed_factorisation_returns(spd):
    """A pivot that fails under the cut (A'_kk = A_kk - 1.5 L_kk^2 in the middle of the matrix, test_gpu_general_spd's construction): schur_factor reports
    it through cholamd_factor_info, and schur, condense and expand return (numbers without meaning), never hang."""
    import torch
    import cholesky_amd as ca
    Sp = spd("g12_full")
    P = Sp.plan
    k, pos = 1, Sp.n // 2
    assert pos < P.n - P.schur_size(k), "the failing pivot lies under the cut"
    host = P.fill_host()
    lbl, off = Sp.sep_of(pos)
    blk = P.blocks[(P.blocks[:, 0] == lbl) & (P.blocks[:, 1] == lbl)][0]
    j = pos - off
    idx = int(blk[7]) + j + j * int(blk[6])
    assert host[idx] == Sp.PAP[pos, pos]
    host[idx] = Sp.PAP[pos, pos] - 1.5 * Sp.Ld[pos, pos] ** 2
    dev = ca.Device(P, 0)
    bad = torch.from_numpy(host).cuda()
    dev.schur_factor(bad, k)
    dev.sync()
    info = dev.info()
    assert info[0] > 0 and info[1] == lbl
    S = dev.schur(bad, k)
    w, g = dev.schur_condense(bad, k, torch.from_numpy(Sp.rhs).cuda())
    dev.schur_expand(bad, k, w, torch.zeros_like(g))
    dev.sync()
    assert tuple(S.shape) == (P.schur_size(k),) * 2 and dev.info() == info


def test_cli_schur(tmp_path):
    case, k = "lapl_400x400", 2
    m, o, c, _ = case_paths(case)
    out = tmp_path / "schur.mtx"
    r = subprocess.run([BIN, "-i", m, "-s", o, "-c", c, "--schur", str(k), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Saving Schur complement" in r.stdout
    with open(out) as f:
        assert f.readline().strip() == "%%MatrixMarket matrix array real general"
        rows, cols = (int(v) for v in f.readline().split())
        vals = np.array([float(v) for v in f.read().split()])
    R = refs(case, k)
    plan, _ = get_plan(case)
    assert rows == cols == R["m"] and vals.size == rows * cols
    S = vals.reshape(cols, rows).T
    err = float(np.abs(S - R["S"]).max())
    print(f"--schur {k}: max|S - S_ref| = {err:.3g}")
    assert err <= 1e-12 * np.abs(R["S"]).max()
    dofs = np.loadtxt(str(out) + ".dofs", dtype=np.int64).reshape(-1)
    assert np.array_equal(dofs - 1, plan.schur_dofs(k))
