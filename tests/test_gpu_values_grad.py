"""Gradients with respect to the value array on the GPU: cholamd_values_grad_pairs, cholamd_values_grad_logdet and the autograd layer on top of them
(cholesky_amd.factorize, Factorization.solve / logdet).

The kernels are held to their host restatements bit for bit (test_values_grad_host.py holds those to long double and to central differences).  End to
end, values.grad and B.grad are compared with a dense reference: Lam_ref = reference_solve(T), X_ref = reference_solve(B), Zref = selinv_ref.zref.
  * B.grad = Lam: SPD.forward_error <= SPD.tol_forward(), column by column.
  * values.grad, entry by entry, S = diag(A)^1/2, (i, j) the entry's position, m_k its multiplicity:
      |err_k| <= m_k (2 tol_forward + (2 nrhs + 1) u) sum_c ||S lam_c||_inf ||S x_c||_inf / (s_i s_j)  +  |c| m_k C_SEL (k + 1) u r_i r_j / (s_i s_j)
    the product rule on two solves that are each within the forward-error tolerance (|lam_i| <= ||S lam||_inf / s_i) plus the rounding of the
    2 nrhs-term sum, and selinv_ref's bound on the entry of the inverse; k + 1 = the factor's longest row plus one.  No entry is left out and a value
    that is not finite fails.
Every test prints its largest observed ratio before it asserts (-s)."""
import ctypes as C
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import selinv_ref as sr  # noqa: E402
import spd_inputs as si  # noqa: E402
from conftest import ROOT  # noqa: E402
from test_values_grad_host import INPUTS, NRHS, _with_explicit_zero, in_pattern, orig_reference  # noqa: E402

U = si.U64
_ZREF = {}


@pytest.fixture(scope="module")
def spd(tmp_path_factory):
    return lambda name: si.cached(tmp_path_factory, name)


def zref(S, name):
    """(Zref in original order, the bound's r in original order) once per input."""
    if name not in _ZREF:
        _ZREF[name] = orig_reference(S, sr.zref(S.PAP, S.Ld))
    return _ZREF[name]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_pairs_on_device(S, name):
    """Device pair sums == host restatement, bit for bit, from guarded buffers with ld > n; inputs unchanged, guards intact, two calls the same bits."""
    import cholesky_amd as ca
    from guarded import Guarded
    plan = S.plan
    n, nz = S.n, plan.nz
    dev = ca.Device(plan, 0)
    rng = np.random.default_rng(21)
    gc.collect()                                                                           # (device objects of earlier tests go now, not inside the loop)
    live = None
    for k in NRHS:
        Ph, Qh = rng.standard_normal((n, k)), rng.standard_normal((n, k)) * 10.0 ** rng.uniform(-3, 3, (n, 1))
        P, Q, g = Guarded(n, k, ld=n + 3, values=Ph), Guarded(n, k, ld=n + 7, values=Qh), Guarded(nz)
        snap = P.snapshot(), Q.snapshot()
        assert np.isnan(g.numpy()).all()                                                   # beta == 0 must not read it
        dev.values_grad_pairs(P.t, Q.t, out=g.t)
        dev.sync()
        want = plan.values_grad_pairs_host(Ph, Qh, ldp=n + 3, ldq=n + 7)
        got = g.numpy()
        assert np.isfinite(got).all() and np.array_equal(bits(got), bits(want)), (name, k)
        g2 = Guarded(nz, values=np.full(nz, -5.0))
        dev.values_grad_pairs(P.t, Q.t, out=g2.t)
        dev.sync()
        assert np.array_equal(bits(g2.numpy()), bits(got))                                 # the same bits again, whatever g held
        g0 = rng.standard_normal(nz)
        g3 = Guarded(nz, values=g0)
        dev.values_grad_pairs(P.t, Q.t, alpha=0.5, beta=2.0, out=g3.t)                     # accumulate
        dev.values_grad_pairs(P.t, P.t, alpha=-1.0, out=g2.t)                              # P is Q: the quadratic form
        dev.sync()
        assert np.array_equal(bits(g3.numpy()), bits(plan.values_grad_pairs_host(Ph, Qh, 0.5, 2.0, g=g0, ldp=n + 3, ldq=n + 7)))
        assert np.array_equal(bits(g2.numpy()), bits(plan.values_grad_pairs_host(Ph, Ph, -1.0, ldp=n + 3, ldq=n + 3)))
        P.assert_unchanged(snap[0], "P")
        Q.assert_unchanged(snap[1], "Q")
        for b, what in ((g, "g"), (g2, "g2"), (g3, "g3")):
            b.assert_guards(what)
        if live is None:
            live = dev.L.cholamd_debug_live_buffers()                                      # the entry list went to the device at the first call ...
        assert dev.L.cholamd_debug_live_buffers() == live                                  # ... and later calls allocate nothing


@pytest.mark.parametrize("name", INPUTS)
def test_device_pair_sums_equal_the_host_restatement(name, spd):
    check_pairs_on_device(spd(name), name)


def poison_child():
    """Runs in a child process with CHOLAMD_POISON=1: the same checks with the library's own buffers poisoned."""
    import tempfile
    assert os.environ.get("CHOLAMD_POISON") == "1"
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("lapl_25x25", "g7_ragged"):
            check_pairs_on_device(si.make(tmp, name), name)
        S = si.make(tmp, "lapl_400x400")
        check_logdet_on_device(S, "lapl_400x400 poisoned")
    print("poison child ok")


def test_poisoned_library_buffers():
    env = dict(os.environ, CHOLAMD_POISON="1")
    code = f"import sys; sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); import conftest, test_gpu_values_grad as t; t.poison_child()"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0 and "poison child ok" in r.stdout, r.stdout + r.stderr


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


def check_logdet_on_device(S, name):
    from guarded import Guarded
    plan = S.plan
    dev, arena = _factor(plan)
    z = dev.selinv(arena)
    v = dev.selinv_entries(z).cpu().numpy()
    g = Guarded(plan.nz)
    dev.values_grad_logdet(z, out=g.t)
    dev.sync()
    got = g.numpy()
    g.assert_guards("g")
    row, col = plan.entries()
    m = np.where(row == col, 1.0, 2.0)
    inpat = in_pattern(plan)
    assert np.array_equal(np.isnan(v), ~inpat)
    assert np.array_equal(bits(got[inpat]), bits(m[inpat] * v[inpat]))                     # m_k times selinv_entries, bit for bit
    assert (got[~inpat] == 0.0).all() and np.isfinite(got).all()                           # 0.0 where selinv_entries writes NaN
    assert np.array_equal(bits(got), bits(plan.values_grad_logdet_host(z.cpu().numpy())))  # the host restatement
    g0 = np.random.default_rng(4).standard_normal(plan.nz)
    g2 = Guarded(plan.nz, values=g0)
    dev.values_grad_logdet(z, alpha=-0.5, beta=3.0, out=g2.t)
    dev.sync()
    assert np.array_equal(bits(g2.numpy()), bits(plan.values_grad_logdet_host(z.cpu().numpy(), -0.5, 3.0, g=g0)))
    assert (g2.numpy()[~inpat] == 3.0 * g0[~inpat]).all()
    Zo, r = zref(S, name)
    i, j = row[inpat], col[inpat]
    q = float(np.max(np.abs(got[inpat] / m[inpat] - Zo[i, j]) * S.s[i] * S.s[j] / ((S.k + 1) * U * r[i] * r[j])))
    print(f"logdet terms gpu {name}: nz = {plan.nz}, outside the pattern = {int((~inpat).sum())}, max ratio = {q:.3g} (bound {sr.C_SEL})")
    assert q <= sr.C_SEL


@pytest.mark.parametrize("name", ["lapl_25x25", "lapl_400x400", "g7_ragged", "tree_over"])
def test_logdet_terms_on_the_device(name, spd):
    check_logdet_on_device(spd(name), name)


def test_logdet_terms_with_an_entry_outside_the_pattern(tmp_path):
    S, k = _with_explicit_zero(tmp_path)
    assert not in_pattern(S.plan)[k]
    check_logdet_on_device(S, "subset with an explicit zero")


# ---- end to end through autograd ----------------------------------------------------------------------------------------------------------------
def _values(S):
    import torch
    row, col = S.plan.entries()
    return torch.from_numpy(np.ascontiguousarray(S.A[row, col])).cuda()


def check_end_to_end(S, name, nrhs, c=0.75, opts=None):
    import cholesky_amd as ca
    import torch
    plan = S.plan
    n = S.n
    rng = np.random.default_rng(100 + nrhs)
    Bh, Th = S.s[:, None] * rng.standard_normal((n, nrhs)), S.s[:, None] * rng.standard_normal((n, nrhs))
    dev = ca.Device(plan, 0)
    for o, val in (opts or {}).items():
        dev.set_option(o, val)
    values = _values(S).requires_grad_(True)
    B = torch.from_numpy(Bh).cuda().requires_grad_(True)                                   # torch's row-major (n, nrhs)
    T = torch.from_numpy(Th).cuda()
    fac = ca.factorize(dev, values)
    X = fac.solve(B)
    assert X.shape == B.shape
    loss = (T * X).sum() + c * fac.logdet()
    loss.backward()
    torch.cuda.synchronize()
    gv, gB = values.grad.cpu().numpy(), B.grad.cpu().numpy()
    assert gv.shape == (plan.nz,) and gB.shape == (n, nrhs) and np.isfinite(gv).all() and np.isfinite(gB).all()
    # the dense reference
    Lam, Xr = S.reference_solve(Th), S.reference_solve(Bh)
    Zo, r = zref(S, name)
    tol = S.tol_forward()
    fe = max(S.forward_error(gB[:, q], Lam[:, q]) for q in range(nrhs))
    fx = max(S.forward_error(X.detach().cpu().numpy()[:, q], Xr[:, q]) for q in range(nrhs))
    row, col = plan.entries()
    m = np.where(row == col, 1.0, 2.0)
    Ll, Xl = Lam.astype(np.longdouble), Xr.astype(np.longdouble)
    pair = (Ll[row] * Xl[col]).sum(axis=1) + np.where(row != col, (Ll[col] * Xl[row]).sum(axis=1), 0)
    ref = -pair + np.longdouble(c) * m * Zo[row, col]
    w = float((np.abs(S.s[:, None] * Lam).max(axis=0) * np.abs(S.s[:, None] * Xr).max(axis=0)).sum())
    ss = S.s[row] * S.s[col]
    bound = m * (2 * tol + (2 * nrhs + 1) * U) * w / ss + abs(c) * m * sr.C_SEL * (S.k + 1) * U * r[row] * r[col] / ss
    err = np.abs(gv.astype(np.longdouble) - ref).astype(np.float64)
    q = float((err / bound).max())
    print(f"autograd {name} nrhs = {nrhs}: n = {n}, nz = {plan.nz}, forward error X / B.grad = {fx:.3g} / {fe:.3g} (tol {tol:.3g}), values.grad max err / bound = {q:.3g}")
    assert fx <= tol and fe <= tol
    assert len(err) == plan.nz and (err <= bound).all(), (name, nrhs, q)
    return gv


@pytest.mark.parametrize("nrhs", [1, 5, 33])
@pytest.mark.parametrize("name", ["lapl_400x400", "g7_ragged", "tree_over"])
def test_autograd_end_to_end(name, nrhs, spd):
    check_end_to_end(spd(name), name, nrhs)


def test_autograd_end_to_end_on_a_badly_scaled_matrix(spd):
    check_end_to_end(spd("lapl_3375_scaled"), "lapl_3375_scaled", 5, c=-1.5)


def test_layouts_and_flags(spd):
    """One Factorization (deterministic solves, so that equal inputs give equal bits), B in every layout, every combination of requires_grad."""
    import cholesky_amd as ca
    import torch
    S = spd("lapl_400x400")
    n, k = S.n, 3
    dev = ca.Device(S.plan, 0)
    dev.set_option("solve_deterministic", 1)
    dev.set_option("solve_deterministic_block", 1)
    rng = np.random.default_rng(31)
    Bh, Th = S.s[:, None] * rng.standard_normal((n, k)), S.s[:, None] * rng.standard_normal((n, k))
    T = torch.from_numpy(Th).cuda()
    values = _values(S).requires_grad_(True)
    fac = ca.factorize(dev, values)
    Lam, tol = S.reference_solve(Th), S.tol_forward()

    def run(B, fac=fac, logdet=0.0):
        """(values.grad, B.grad) of (T * solve(B)).sum() + logdet * logdet(), the gradients cleared first."""
        fac.values.grad = None
        loss = (T * fac.solve(B)).sum()
        if logdet:
            loss = loss + logdet * fac.logdet()
        if loss.requires_grad:
            loss.backward()
        torch.cuda.synchronize()
        return fac.values.grad, (B.grad if B.is_leaf else None)

    # torch's row-major (n, k): the run the others are compared with
    B0 = torch.from_numpy(Bh).cuda().requires_grad_(True)
    assert B0.is_contiguous()
    gv0, gB0 = run(B0)
    assert gv0.shape == (S.plan.nz,) and gB0.shape == (n, k)
    assert max(S.forward_error(gB0.cpu().numpy()[:, q], Lam[:, q]) for q in range(k)) <= tol
    # column-major
    B1 = torch.from_numpy(np.ascontiguousarray(Bh.T)).cuda().T.detach().requires_grad_(True)
    assert B1.stride() == (1, n)
    gv1, gB1 = run(B1)
    assert torch.equal(gv1, gv0) and torch.equal(gB1, gB0)
    # a non-contiguous slice of a wider array
    wide = torch.zeros((n, 2 * k + 1), dtype=torch.float64, device="cuda")
    wide[:, 1::2] = torch.from_numpy(Bh).cuda()
    wide.requires_grad_(True)
    Bs = wide[:, 1::2]
    assert not Bs.is_contiguous()
    gv2, _ = run(Bs)
    assert torch.equal(gv2, gv0) and torch.equal(wide.grad[:, 1::2], gB0) and bool((wide.grad[:, 0::2] == 0).all())
    # 1-D: column 0 alone (the deterministic block solve: a column's bits do not depend on the other columns)
    b = torch.from_numpy(np.ascontiguousarray(Bh[:, 0])).cuda().requires_grad_(True)
    fac.values.grad = None
    x = fac.solve(b)
    assert x.shape == (n,)
    (T[:, 0] * x).sum().backward()
    assert b.grad.shape == (n,)
    assert S.forward_error(b.grad.cpu().numpy(), Lam[:, 0]) <= tol and S.forward_error(x.detach().cpu().numpy(), S.reference_solve(Bh[:, 0])) <= tol
    # B without a gradient: values.grad alone, the same bits
    gv3, gB3 = run(torch.from_numpy(Bh).cuda())
    assert gB3 is None and torch.equal(gv3, gv0)
    # values without a gradient: B.grad alone (a second factorisation on the same device object and arena)
    plain = ca.factorize(dev, _values(S), arena=fac.arena)
    B4 = torch.from_numpy(Bh).cuda().requires_grad_(True)
    gv4, gB4 = run(B4, fac=plain)
    assert gv4 is None and max(S.forward_error(gB4.cpu().numpy()[:, q], Lam[:, q]) for q in range(k)) <= tol
    gv5, gB5 = run(torch.from_numpy(Bh).cuda(), fac=plain)
    assert gv5 is None and gB5 is None
    # solve and logdet accumulate into one values.grad; release() drops the Z arena and the next backward brings it back
    fac = ca.factorize(dev, values, arena=fac.arena)
    gv0, _ = (g.clone() if g is not None else None for g in run(torch.from_numpy(Bh).cuda(), fac=fac))
    ld = fac.logdet()
    assert ld.shape == () and ld.dtype == torch.float64 and ld.is_cuda
    assert abs(float(ld.detach()) - float(np.linalg.slogdet(S.A)[1])) <= 1e-10 * abs(float(ld.detach()))
    values.grad = None
    assert fac._z is None
    (2.0 * ld).backward()
    only_logdet = values.grad.clone()
    assert fac._z is not None
    gv6, _ = run(torch.from_numpy(Bh).cuda(), fac=fac, logdet=2.0)
    assert torch.equal(gv6, gv0 + only_logdet)
    fac.release()
    assert fac._z is None
    values.grad = None
    (2.0 * fac.logdet()).backward()
    assert fac._z is not None and torch.equal(values.grad, only_logdet)
    # refused inputs
    with pytest.raises(ValueError):
        fac.solve(torch.zeros((n + 1, 2), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        fac.solve(torch.zeros((n, 2), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        ca.factorize(dev, _values(S)[:-1])
    with pytest.raises(ValueError):
        ca.factorize(dev, S.A[S.plan.entries()])


def test_determinism_with_the_deterministic_solves(spd):
    """Two forward-plus-backward passes on one Factorization give the same bits of values.grad and B.grad."""
    import cholesky_amd as ca
    import torch
    S = spd("g7_ragged")
    n, k = S.n, 33
    dev = ca.Device(S.plan, 0)
    dev.set_option("solve_deterministic", 1)
    dev.set_option("solve_deterministic_block", 1)
    rng = np.random.default_rng(41)
    T = torch.from_numpy(S.s[:, None] * rng.standard_normal((n, k))).cuda()
    values = _values(S).requires_grad_(True)
    fac = ca.factorize(dev, values)
    got = []
    for _ in range(2):
        values.grad = None
        B = torch.from_numpy(S.s[:, None] * np.random.default_rng(42).standard_normal((n, k))).cuda().requires_grad_(True)
        ((T * fac.solve(B)).sum() - 0.5 * fac.logdet()).backward()
        torch.cuda.synchronize()
        got.append((values.grad.cpu().numpy().copy(), B.grad.cpu().numpy().copy()))
        fac.release()                                                                      # the second pass runs the selected inversion again
    assert np.isfinite(got[0][0]).all()
    assert np.array_equal(bits(got[0][0]), bits(got[1][0])) and np.array_equal(bits(got[0][1]), bits(got[1][1]))


def test_argument_errors(spd):
    import cholesky_amd as ca
    import torch
    S = spd("lapl_400x400")
    plan = S.plan
    n, nz, na, k = S.n, plan.nz, plan.arena_doubles, 3
    dev = ca.Device(plan, 0)
    L = dev.L
    big = torch.full((nz + k * (n + 2) + 8,), 7.0, dtype=torch.float64, device="cuda")     # g, P and Q cut from one buffer, so that they can overlap
    z = torch.full((na + nz,), 7.0, dtype=torch.float64, device="cuda")
    g = torch.full((nz,), 3.0, dtype=torch.float64, device="cuda")
    P = torch.ones((k, n + 2), dtype=torch.float64, device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + 8 * off)  # noqa: E731
    ld = n + 2

    def pairs(P_=p(P), ldp=ld, Q_=p(P), ldq=ld, nrhs=k, g_=p(g), count=nz, d=dev.h):
        return L.cholamd_values_grad_pairs(d, P_, ldp, Q_, ldq, nrhs, 1.0, 0.0, g_, count, None)

    def logdet(z_=p(z), g_=p(g), count=nz, d=dev.h):
        return L.cholamd_values_grad_logdet(d, z_, 1.0, 0.0, g_, count, None)

    for count in (nz - 1, nz + 1, 0):
        assert pairs(count=count) == -4 and logdet(count=count) == -4
    assert pairs(P_=None) == -4 and pairs(Q_=None) == -4 and pairs(g_=None) == -4 and logdet(z_=None) == -4 and logdet(g_=None) == -4
    assert pairs(nrhs=-1) == -4 and pairs(ldp=n - 1) == -4 and pairs(ldq=n - 1) == -4
    # g inside the full extent (nrhs - 1) ld + n of P or Q (its last element), and just behind it (legal); g inside the Z arena
    ext = (k - 1) * ld + n
    assert pairs(P_=p(big), Q_=p(P), g_=p(big, ext - 1)) == -4 and pairs(P_=p(P), Q_=p(big), g_=p(big, ext - 1)) == -4
    assert pairs(P_=p(big, nz), Q_=p(P), g_=p(big, 1)) == -4                               # g's last element is P's first
    assert logdet(z_=p(z), g_=p(z, na - 1)) == -4 and logdet(z_=p(z, nz - 1), g_=p(z)) == -4
    assert pairs(nrhs=0) == 0 and pairs(nrhs=0, P_=None, Q_=None, g_=None) == 0            # nothing to do, nothing touched
    dev.sync()
    assert bool((g == 3.0).all()) and bool((big == 7.0).all()) and bool((z == 7.0).all())
    assert pairs(P_=p(big), Q_=p(P), g_=p(big, ext)) == 0                                  # g right behind P: accepted, and only g is written
    dev.sync()
    assert bool((big[:ext] == 7.0).all()) and bool((big[ext:ext + nz] != 7.0).all()) and bool((big[ext + nz:] == 7.0).all())
    # a partitioned device object
    part = ca.Device(plan, 0)
    part.set_partition(0, 2)
    assert pairs(d=part.h) == -4 and b"partition" in L.cholamd_last_error()
    assert logdet(d=part.h) == -4
    dev.sync()
    assert bool((g == 3.0).all())
    # the Python mirrors refuse what the library would misread
    with pytest.raises(ValueError):
        dev.values_grad_pairs(P.T[:n], P.T[:n, :2])
    with pytest.raises(ValueError):
        dev.values_grad_pairs(P.T[:n], P.T[:n], beta=1.0)
    with pytest.raises(ValueError):
        dev.values_grad_logdet(z[:na], out=torch.empty(nz + 1, dtype=torch.float64, device="cuda"))


def test_refused_plans_on_the_device(spd, tmp_path):
    import cholesky_amd as ca
    import torch
    from test_values_grad_host import _plan_with_extra
    S = spd("lapl_25x25")
    e = int(np.nonzero(S.row != S.col)[0][0])
    dup = _plan_with_extra(tmp_path, S, int(S.row[e]), int(S.col[e]), 0.25, "dup")
    assert dup.duplicate_entries == 1
    dev = ca.Device(dup, 0)
    P = torch.ones((2, S.n), dtype=torch.float64, device="cuda").T
    g = torch.full((dup.nz,), 3.0, dtype=torch.float64, device="cuda")
    with pytest.raises(ca.CholamdError, match="repeat"):
        dev.values_grad_pairs(P, P, out=g)
    with pytest.raises(ca.CholamdError, match="repeat"):
        dev.values_grad_logdet(dev.new_arena(), out=g)
    dev.sync()
    assert bool((g == 3.0).all())


def test_pivot_failure_raises(spd):
    import cholesky_amd as ca
    S = spd("lapl_400x400")
    dev = ca.Device(S.plan, 0)
    values = _values(S)
    row, col = S.plan.entries()
    d = int(np.nonzero(row == col)[0][len(row) // 7])
    bad = values.clone()
    bad[d] = -bad[d]
    with pytest.raises(ca.CholamdError, match="not positive definite"):
        ca.factorize(dev, bad.requires_grad_(True))
    fac = ca.factorize(dev, values)                                                        # the device object is usable afterwards
    assert np.isfinite(float(fac.logdet()))
