"""Schur condense / expand for many right-hand sides on the GPU (cholamd_schur_condense_nrhs / _expand_nrhs and their _f32 forms) and the device option
schur_deterministic (single-vector and block forms), all through the C ABI.

Inputs (input, k): lapl_400x400 k = 3 (unrelated kept separators, tiles without storage); lapl_3375x3375 k = 1, 2; tree_tiny k = 1, 3 (separators of
1 - 33 columns, pieces under a 16-row tile); tree_over k = 1 (leaves of 257 and 273 columns: two spans under the cut; root of 193), k = 2 ("tiles"
couplings into kept grandparents); tree_at k = 1 (the same sizes minus one).  Column counts and padding (nrhs, ld - rows): (1, 0) (5, 0) (32, 0) (33, 0)
(40, 3): under, at and over one chunk, a second chunk under the column-by-column threshold (1 column) and over it (8 columns).

References, computed once per (input, k) and shared: numpy on the permuted dense A (I = [0, t0), T = [t0, n)): g_ref = b_T - A_TI solve(A_II, b_I); the
expanded X with XT = solve(S, G), S from dev.schur; cholamd_solve on the completed factor.  Gates (none measured from the code under test), per column:
  * fixtures: |G - g_ref|_max <= 1e-12 |g_ref|_max, residual <= 1e-10, |X - x_solve|_max <= 1e-10 |x_solve|_max (test_condense_and_expand's);
  * trees: each gate becomes max(gate, 100 x the relative difference of two CPU routes to the same quantity) -- the rule of test_general_spd_inputs:
    g by an LU solve of A_II and by the Cholesky factor of P A P^T; x by an LU solve of A and by that factor; the residual of those two x;
  * fp32 arena: error of X against the fp64 solve <= 10 x what solve_f32 loses against solve on the same column (test_fp32_arena's);
  * "to rounding" between two paths: 1e-12 of the largest element, the gate of a factor entry; "the same bits": torch.equal.
Every test prints what it measured before it asserts (-s)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tree_inputs  # noqa: E402
from conftest import CASES, ROOT, case_paths  # noqa: E402

SHAPES = [("lapl_400x400", 3), ("lapl_3375x3375", 1), ("lapl_3375x3375", 2), ("tree_tiny", 1), ("tree_tiny", 3), ("tree_over", 1), ("tree_over", 2),
          ("tree_at", 1)]
IDS = [f"{c}-k{k}" for c, k in SHAPES]
COLS = [(1, 0), (5, 0), (32, 0), (33, 0), (40, 3)]
KMAX = 40
SENT = -7.0
_BASE, _CTX = {}, {}


class Base:
    """plan, permuted dense A, its Cholesky factor and a block of KMAX right-hand sides of one input."""

    def __init__(self, name, tmp):
        import cholesky_amd as ca
        self.name, self.tree = name, name not in CASES
        if not self.tree:
            files = case_paths(name)
            self.plan = ca.Plan(*files[:3])
            b = np.asarray(ca.plan.read_vector(files[3], self.plan.n), dtype=np.float64)
            D = self.plan.arena_to_dense(self.plan.fill_host())
            self.A = np.tril(D) + np.tril(D, -1).T
            self.Ld = None
        else:
            S = tree_inputs.cached(tmp, name)
            self.plan, b, self.A, self.Ld = S.plan, np.asarray(S.rhs, dtype=np.float64), np.asarray(S.PAP, dtype=np.float64), np.asarray(S.Ld, dtype=np.float64)
        P = self.plan
        s = np.empty(P.n)
        s[P.perm] = np.sqrt(np.diag(self.A))
        self.B = s[:, None] * np.random.default_rng(53).standard_normal((P.n, KMAX))
        self.B[:, 0] = b
        self.B.setflags(write=False)


class Ctx:
    """One (input, k): the device object, the arenas eliminated down to level k (fp64, fp32), S, the references and the gates."""

    def __init__(self, base, k):
        import scipy.linalg as sl
        import torch
        import cholesky_amd as ca
        P, A = base.plan, base.A
        self.base, self.k, self.plan = base, k, P
        self.m = m = P.schur_size(k)
        self.t0 = t0 = P.n - m
        Bp = base.B[P.perm]
        g1 = Bp[t0:] - A[t0:, :t0] @ np.linalg.solve(A[:t0, :t0], Bp[:t0])
        self.Gref = g1
        self.gate_g, self.gate_x, self.gate_r = np.full(KMAX, 1e-12), np.full(KMAX, 1e-10), np.full(KMAX, 1e-10)
        if base.tree:                                                # the two-CPU-routes rule
            Ld = base.Ld
            y = sl.solve_triangular(Ld[:t0, :t0], Bp[:t0], lower=True)
            g2 = Bp[t0:] - Ld[t0:, :t0] @ y
            x1, x2 = np.linalg.solve(A, Bp), sl.cho_solve((Ld, True), Bp)
            nb = np.linalg.norm(Bp, axis=0)
            route_g = np.abs(g1 - g2).max(axis=0) / np.abs(g1).max(axis=0)
            route_x = np.abs(x1 - x2).max(axis=0) / np.abs(x1).max(axis=0)
            route_r = np.maximum(np.linalg.norm(Bp - A @ x1, axis=0), np.linalg.norm(Bp - A @ x2, axis=0)) / nb
            self.gate_g, self.gate_x, self.gate_r = (np.maximum(g, 100.0 * r) for g, r in ((self.gate_g, route_g), (self.gate_x, route_x), (self.gate_r, route_r)))
        self.dev = dev = ca.Device(P, 0)
        self.arena = dev.new_arena()
        dev.fill(self.arena)
        dev.schur_factor(self.arena, k)
        self.a32 = dev.new_arena_f32()
        dev.fill_f32(self.a32)
        dev.factor_levels_f32(self.a32, P.levels - 1, k)
        dev.sync()
        assert dev.info() == (0, 0)
        self.S = dev.schur(self.arena, k).cpu().numpy()
        self.dB = torch.from_numpy(np.asfortranarray(base.B).T.copy()).cuda().T      # n x KMAX, column-major
        # the yardsticks: cholamd_solve on the completed factor, cholamd_solve_f32 on the fp32 factor, column by column
        full = self.arena.clone()
        dev.factor_levels(full, k - 1, 0)
        full32 = dev.new_arena_f32()
        dev.fill_f32(full32)
        dev.factor_f32(full32)
        X64 = torch.empty((KMAX, P.n), dtype=torch.float64, device="cuda")
        X32 = torch.empty_like(X64)
        for j in range(KMAX):
            dev.solve(full, self.dB[:, j].contiguous(), X64[j])
            dev.solve_f32(full32, self.dB[:, j].contiguous(), X32[j])
        dev.sync()
        assert dev.info() == (0, 0)
        self.Xs = X64.cpu().numpy().T
        self.yard = np.abs(X32.cpu().numpy().T - self.Xs).max(axis=0) / np.abs(self.Xs).max(axis=0)
        self.nanpieces = None

    def arena_of(self, f32):
        return self.a32 if f32 else self.arena

    def pieces(self):
        """The arena offsets of every schur_list(k) piece, on the device."""
        import torch
        if self.nanpieces is None:
            offs = [(off + np.arange(rows)[:, None] + np.arange(cols)[None, :] * ld).ravel() for off, ld, rows, cols, _, _, _ in self.plan.schur_list(self.k)]
            self.nanpieces = torch.from_numpy(np.unique(np.concatenate(offs))).cuda()
        return self.nanpieces

    def xt_of(self, G):
        """XT = solve(S, G) on the host, back as a column-major device block."""
        import torch
        xt = np.linalg.solve(self.S, G.cpu().numpy())
        return torch.from_numpy(np.ascontiguousarray(xt.T)).cuda().T


@pytest.fixture
def ctx(tmp_path_factory):
    def get(name, k):
        if name not in _BASE:
            _BASE[name] = Base(name, tmp_path_factory)
        if (name, k) not in _CTX:
            _CTX[name, k] = Ctx(_BASE[name], k)
        c = _CTX[name, k]
        c.dev.set_option("schur_deterministic", 0)
        return c
    return get


@pytest.fixture(autouse=True)
def environment(monkeypatch):
    for v in ("CHOLAMD_SCHUR_DETERMINISTIC", "CHOLAMD_SOLVE_DETERMINISTIC", "CHOLAMD_SOLVE_DETERMINISTIC_BLOCK", "CHOLAMD_SOLVE_REFERENCE_SHAPE", "CHOLAMD_POISON"):
        monkeypatch.delenv(v, raising=False)


def padded(rows, cols, pad, extra_cols=0, fill=SENT):
    """(buffer, view): a column-major rows x cols view with leading dimension rows + pad inside a sentinel-filled buffer of cols + extra_cols columns."""
    import torch
    buf = torch.full((cols + extra_cols, rows + pad), fill, dtype=torch.float64, device="cuda")
    return buf, buf.T[:rows, :cols]


def block_in(src, rows, cols, pad):
    """A column-major copy of src[:, :cols] with leading dimension rows + pad."""
    buf, view = padded(rows, cols, pad)
    view.copy_(src[:, :cols])
    return view


def run_block(c, f32, nrhs, pad, B=None):
    """(W, G, XT, X) of the block calls on the first nrhs columns."""
    P, dev, a = c.plan, c.dev, c.arena_of(f32)
    Bv = block_in(c.dB if B is None else B, P.n, nrhs, pad)
    _, W = padded(P.n, nrhs, pad)
    _, G = padded(c.m, nrhs, pad)
    _, X = padded(P.n, nrhs, pad)
    dev.schur_condense_nrhs(a, c.k, Bv, W=W, G=G)
    XT = block_in(c.xt_of(G), c.m, nrhs, pad)
    dev.schur_expand_nrhs(a, c.k, W, XT, X=X)
    dev.sync()
    return W, G, XT, X


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name,k", SHAPES, ids=IDS)
def test_against_the_reference_both_paths(name, k, f32, ctx):
    c = ctx(name, k)
    P, dev = c.plan, c.dev
    Bp = c.base.B[P.perm]
    nb = np.linalg.norm(Bp, axis=0)
    for det in (0, 1):
        dev.set_option("schur_deterministic", det)
        for nrhs, pad in COLS:
            W, G, XT, X = run_block(c, f32, nrhs, pad)
            Gh, Xh = G.cpu().numpy(), X.cpu().numpy()
            assert np.isfinite(Gh).all() and np.isfinite(Xh).all()
            assert np.array_equal(W.cpu().numpy()[c.t0:], Gh), "the tail of W is G"
            xerr = np.abs(Xh - c.Xs[:, :nrhs]).max(axis=0) / np.abs(c.Xs[:, :nrhs]).max(axis=0)
            tag = f"{name} k = {k} {'fp32' if f32 else 'fp64'} det = {det} nrhs = {nrhs} pad = {pad}"
            if f32:
                ratio = xerr / c.yard[:nrhs]
                print(f"{tag}: worst error of X = {xerr.max():.3g}, worst ratio to the same column's solve_f32 loss = {ratio.max():.3g} (bound 10)")
                assert (c.yard[:nrhs] > 0).all() and (ratio <= 10.0).all()
                continue
            gerr = np.abs(Gh - c.Gref[:, :nrhs]).max(axis=0) / np.abs(c.Gref[:, :nrhs]).max(axis=0)
            res = np.linalg.norm(Bp[:, :nrhs] - c.base.A @ Xh[P.perm], axis=0) / nb[:nrhs]
            print(f"{tag}: worst ratio to its gate: g {np.max(gerr / c.gate_g[:nrhs]):.3g}, residual {np.max(res / c.gate_r[:nrhs]):.3g}, "
                  f"x vs solve {np.max(xerr / c.gate_x[:nrhs]):.3g}; worst g error {gerr.max():.3g}, residual {res.max():.3g}, x error {xerr.max():.3g}")
            assert (gerr <= c.gate_g[:nrhs]).all() and (res <= c.gate_r[:nrhs]).all() and (xerr <= c.gate_x[:nrhs]).all()


@pytest.mark.parametrize("name,k", [("lapl_400x400", 3), ("tree_over", 1)], ids=["lapl_400-k3", "tree_over-k1"])
def test_interchange_with_the_single_vector_calls(name, k, ctx):
    """A column of W is a valid w for schur_expand, and a w is a valid column of W; both agree with the block result to rounding."""
    import torch
    c = ctx(name, k)
    P, dev = c.plan, c.dev
    for det in (0, 1):
        dev.set_option("schur_deterministic", det)
        for f32 in (False, True):
            a = c.arena_of(f32)
            W, G, XT, X = run_block(c, f32, 33, 0)
            scale = float(X.abs().max())
            for j in (0, 17, 32):
                xj = dev.schur_expand(a, c.k, W[:, j].contiguous(), XT[:, j].contiguous())
                w1, g1 = dev.schur_condense(a, c.k, c.dB[:, j].contiguous())
                W2 = W.clone(memory_format=torch.preserve_format)
                W2[:, j] = w1
                X2 = dev.schur_expand_nrhs(a, c.k, W2, XT)
                dev.sync()
                e1 = float((xj - X[:, j]).abs().max()) / scale
                e2 = float((X2[:, j] - X[:, j]).abs().max()) / scale
                e3 = float((w1 - W[:, j]).abs().max()) / float(W.abs().max())
                print(f"interchange {name} k = {k} det = {det} f32 = {f32} column {j}: single expand of W's column {e1:.3g}, block expand of a single w {e2:.3g}, w {e3:.3g}")
                assert e1 <= 1e-12 and e2 <= 1e-12 and e3 <= 1e-12
                keep = [i for i in range(33) if i != j]
                if det:
                    assert torch.equal(X2[:, keep], X[:, keep]), "the other columns keep their bits"


def det_outputs(c, dev, f32, nrhs=33, pad=0):
    """Everything the option covers, on `dev`: block (W, G, X) and single-vector (w, g, x) of column 5."""
    a = c.arena_of(f32)
    P = c.plan
    Bv = block_in(c.dB, P.n, nrhs, pad)
    _, W = padded(P.n, nrhs, pad)
    _, G = padded(c.m, nrhs, pad)
    _, X = padded(P.n, nrhs, pad)
    dev.schur_condense_nrhs(a, c.k, Bv, W=W, G=G)
    XT = block_in(c.xt_fixed[:, :nrhs], c.m, nrhs, pad)
    dev.schur_expand_nrhs(a, c.k, W, XT, X=X)
    w, g = dev.schur_condense(a, c.k, c.dB[:, 5].contiguous())
    x = dev.schur_expand(a, c.k, w, c.xt_fixed[:, 5].contiguous())
    dev.sync()
    return [t.contiguous() for t in (W, G, X, w, g, x)]


def fixed_xt(c):
    """An XT that does not depend on any run: solve(S, g_ref)."""
    import torch
    if not hasattr(c, "xt_fixed"):
        c.xt_fixed = torch.from_numpy(np.ascontiguousarray(np.linalg.solve(c.S, c.Gref).T)).cuda().T
    return c.xt_fixed


BITS = [("lapl_400x400", 3), ("lapl_3375x3375", 1), ("tree_tiny", 3), ("tree_over", 1), ("tree_over", 2)]


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name,k", BITS, ids=[f"{c}-k{k}" for c, k in BITS])
def test_the_same_bits(name, k, f32, ctx):
    """(a): two calls, two device objects, ld > rows."""
    import torch
    import cholesky_amd as ca
    c = ctx(name, k)
    fixed_xt(c)
    c.dev.set_option("schur_deterministic", 1)
    first = det_outputs(c, c.dev, f32)
    again = det_outputs(c, c.dev, f32)
    wide = det_outputs(c, c.dev, f32, pad=3)
    dev2 = ca.Device(c.plan, 0)
    dev2.set_option("schur_deterministic", 1)
    other = det_outputs(c, dev2, f32)
    for what, outs in (("a second call", again), ("ld > rows", wide), ("a second device object", other)):
        for tag, p, q in zip("WGXwgx", first, outs):
            assert bool(torch.isfinite(p).all()) and torch.equal(p, q), (name, k, what, tag)


def poison_child(path):
    """Runs in a child process with CHOLAMD_POISON=1: the bits of the deterministic paths equal those the parent saved from a clean device object."""
    import torch
    assert os.environ.get("CHOLAMD_POISON") == "1"
    saved = np.load(path)

    class TF:
        def mktemp(self, *_a, **_k):
            import pathlib
            import tempfile
            return pathlib.Path(tempfile.mkdtemp())
    for name, k in POISON:
        if name not in _BASE:
            _BASE[name] = Base(name, TF())
        c = Ctx(_BASE[name], k)
        fixed_xt(c)
        c.dev.set_option("schur_deterministic", 1)
        for f32 in (False, True):
            outs = det_outputs(c, c.dev, f32, pad=3)
            for tag, t in zip("WGXwgx", outs):
                ref = saved[f"{name}-{k}-{int(f32)}-{tag}"]
                assert np.isfinite(ref).all() and np.array_equal(t.cpu().numpy(), ref), (name, k, f32, tag)
        assert bool(torch.isfinite(c.arena).all())
    print("poison child ok")


POISON = [("lapl_400x400", 3), ("tree_over", 1)]


def test_the_same_bits_on_a_poisoned_device_object(ctx, tmp_path):
    """(a): a device object created under CHOLAMD_POISON=1 (NaN-filled, guarded scratch) returns the bits of a clean one."""
    out = {}
    for name, k in POISON:
        c = ctx(name, k)
        fixed_xt(c)
        c.dev.set_option("schur_deterministic", 1)
        for f32 in (False, True):
            for tag, t in zip("WGXwgx", det_outputs(c, c.dev, f32, pad=3)):
                out[f"{name}-{k}-{int(f32)}-{tag}"] = t.cpu().numpy()
    path = str(tmp_path / "bits.npz")
    np.savez(path, **out)
    env = dict(os.environ, CHOLAMD_POISON="1")
    code = f"import sys; sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); import conftest, test_gpu_schur_nrhs as t; t.poison_child({path!r})"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0 and "poison child ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name,k", BITS, ids=[f"{c}-k{k}" for c, k in BITS])
def test_columns_are_independent(name, k, f32, ctx):
    """(b): a column alone, at position 0, at position 17 and in the second chunk has the same bits; a NaN column next to it does not reach it."""
    import torch
    c = ctx(name, k)
    P, dev, a = c.plan, c.dev, c.arena_of(f32)
    xt_all = fixed_xt(c)
    dev.set_option("schur_deterministic", 1)
    j = 9
    b1, t1 = c.dB[:, j:j + 1], xt_all[:, j:j + 1]
    W1, G1 = dev.schur_condense_nrhs(a, c.k, block_in(b1, P.n, 1, 0))
    X1 = dev.schur_expand_nrhs(a, c.k, W1, block_in(t1, c.m, 1, 0))
    dev.sync()
    assert bool(torch.isfinite(W1).all() and torch.isfinite(X1).all())
    for pos, nrhs in ((0, 5), (17, 32), (35, 40)):
        order = [i for i in range(nrhs) if i != j][:nrhs - 1]
        order.insert(pos, j)
        Bq, Tq = c.dB[:, order], xt_all[:, order]
        for nan_at in (None, pos - 1 if pos else pos + 1):
            Bn, Tn = block_in(Bq, P.n, nrhs, 0), block_in(Tq, c.m, nrhs, 0)
            if nan_at is not None:
                Bn[:, nan_at] = float("nan")
                Tn[0, nan_at] = float("nan")
            W, G = dev.schur_condense_nrhs(a, c.k, Bn)
            Wn = W.clone(memory_format=torch.preserve_format)
            if nan_at is not None:
                assert bool(torch.isnan(W[:, nan_at]).any()), "the NaN column stays NaN"
            X = dev.schur_expand_nrhs(a, c.k, Wn, Tn)
            dev.sync()
            tag = (name, k, f32, pos, nrhs, nan_at)
            assert torch.equal(W[:, pos], W1[:, 0]) and torch.equal(G[:, pos], G1[:, 0]) and torch.equal(X[:, pos], X1[:, 0]), tag


@pytest.mark.parametrize("name,k", [("lapl_400x400", 3), ("tree_tiny", 3), ("tree_over", 2)], ids=["lapl_400-k3", "tree_tiny-k3", "tree_over-k2"])
def test_s_is_never_read(name, k, ctx):
    """(c): NaN over every schur_list(k) piece of the device arena: all four sweeps of both paths return finite outputs, and under the option the
    bits they return without the NaNs."""
    import torch
    c = ctx(name, k)
    dev = c.dev
    fixed_xt(c)
    clean = {}
    for det in (0, 1):
        dev.set_option("schur_deterministic", det)
        for f32 in (False, True):
            clean[det, f32] = det_outputs(c, dev, f32)
    good = (c.arena, c.a32)
    try:
        c.arena, c.a32 = c.arena.clone(), c.a32.clone()
        idx = c.pieces()
        assert bool(torch.isfinite(c.arena[idx]).any())
        c.arena[idx] = float("nan")
        c.a32[idx] = float("nan")
        for det in (0, 1):
            dev.set_option("schur_deterministic", det)
            for f32 in (False, True):
                outs = det_outputs(c, dev, f32)
                for tag, p, q in zip("WGXwgx", clean[det, f32], outs):
                    assert bool(torch.isfinite(q).all()), (name, k, det, f32, tag)
                    if det:
                        assert torch.equal(p, q), (name, k, f32, tag)
                    else:
                        assert float((p - q).abs().max()) <= 1e-12 * float(p.abs().max()), (name, k, f32, tag)
    finally:
        c.arena, c.a32 = good


def test_caller_memory_and_argument_errors(ctx):
    import torch
    import cholesky_amd as ca
    c = ctx("lapl_400x400", 3)
    P, dev, k, n, m = c.plan, c.dev, c.k, c.plan.n, c.m
    L, h = dev.L, dev.h
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    fixed_xt(c)
    for det in (0, 1):
        dev.set_option("schur_deterministic", det)
        for f32 in (False, True):
            a = c.arena_of(f32)
            for nrhs, pad in ((5, 3), (40, 3), (33, 1)):
                Bv = block_in(c.dB, n, nrhs, 0)
                wb, W = padded(n, nrhs, pad, extra_cols=2)
                gb, G = padded(m, nrhs, pad, extra_cols=2)
                xb, X = padded(n, nrhs, pad, extra_cols=2)
                dev.schur_condense_nrhs(a, k, Bv, W=W, G=G)
                XT = block_in(c.xt_fixed, m, nrhs, 2)
                w0 = wb.clone()
                dev.schur_expand_nrhs(a, k, W, XT, X=X)
                dev.sync()
                assert torch.equal(wb, w0), "the expand wrote W"
                for buf, rows, what in ((wb, n, "W"), (gb, m, "G"), (xb, n, "X")):
                    assert bool((buf[:, rows:] == SENT).all()) and bool((buf[nrhs:] == SENT).all()), (what, "padding rows or columns >= nrhs written")
                    assert bool(torch.isfinite(buf[:nrhs, :rows]).all())
    # the refusals: CHOLAMD_ERR_ARG, nothing written
    dev.set_option("schur_deterministic", 0)
    nrhs = 5
    Bv = block_in(c.dB, n, nrhs, 0)
    W_ok, G_ok = dev.schur_condense_nrhs(c.arena, k, Bv)
    XT_ok = block_in(c.xt_fixed, m, nrhs, 0)
    dev.sync()
    snap = c.arena.clone()
    wb, W = padded(n, nrhs, 0)
    gb, G = padded(m, nrhs, 0)
    xb, X = padded(n, nrhs, 0)
    na = P.arena_doubles
    big = torch.full((na + n * nrhs,), SENT, dtype=torch.float64, device="cuda")
    wg = torch.full((2 * n * nrhs,), SENT, dtype=torch.float64, device="cuda")
    part = ca.Device(P, 0)
    part.set_partition(0, 2)
    for det in (0, 1):
        dev.set_option("schur_deterministic", det)
        part.set_option("schur_deterministic", det)
        for fc, fe, ar in ((L.cholamd_schur_condense_nrhs, L.cholamd_schur_expand_nrhs, c.arena), (L.cholamd_schur_condense_nrhs_f32, L.cholamd_schur_expand_nrhs_f32, c.a32)):
            A_, B_, W_, G_, X_, Wk, Tk = ptr(ar), ptr(Bv), ptr(W), ptr(G), ptr(X), ptr(W_ok), ptr(XT_ok)
            for bad in (0, -1, P.levels, P.levels + 2):
                assert fc(h, A_, bad, B_, n, W_, n, G_, m, nrhs, None) == -4 and fe(h, A_, bad, Wk, n, Tk, m, X_, n, nrhs, None) == -4
            assert fc(None, A_, k, B_, n, W_, n, G_, m, nrhs, None) == -4 and fe(None, A_, k, Wk, n, Tk, m, X_, n, nrhs, None) == -4
            for args in ((None, B_, n, W_, n, G_, m), (A_, None, n, W_, n, G_, m), (A_, B_, n, None, n, G_, m), (A_, B_, n, W_, n, None, m),
                         (A_, B_, n - 1, W_, n, G_, m), (A_, B_, n, W_, n - 1, G_, m), (A_, B_, n, W_, n, G_, m - 1)):
                assert fc(h, args[0], k, *args[1:], nrhs, None) == -4, args
            for args in ((None, Wk, n, Tk, m, X_, n), (A_, None, n, Tk, m, X_, n), (A_, Wk, n, None, m, X_, n), (A_, Wk, n, Tk, m, None, n),
                         (A_, Wk, n - 1, Tk, m, X_, n), (A_, Wk, n, Tk, m - 1, X_, n), (A_, Wk, n, Tk, m, X_, n - 1)):
                assert fe(h, args[0], k, *args[1:], nrhs, None) == -4, args
            assert fc(h, A_, k, B_, n, W_, n, G_, m, -1, None) == -4 and fe(h, A_, k, Wk, n, Tk, m, X_, n, -1, None) == -4
            # nrhs = 0: accepted, nothing touched, whatever the pointers
            assert fc(h, None, k, None, n, None, n, None, m, 0, None) == 0 and fe(h, None, k, None, n, None, m, None, n, 0, None) == 0
            assert fc(h, A_, k, B_, n - 1, W_, n, G_, m, 0, None) == -4
            # overlap over the full (nrhs - 1) ld + rows extents
            half = n * nrhs
            assert fc(h, A_, k, ptr(wg[:half]), n, ptr(wg[half - 1:]), n, G_, m, nrhs, None) == -4              # B and W
            assert fc(h, A_, k, B_, n, ptr(wg[:half]), n, ptr(wg[half - 1:]), m, nrhs, None) == -4              # W and G
            assert fc(h, A_, k, ptr(wg[:half]), n, W_, n, ptr(wg[half - 1:]), m, nrhs, None) == -4              # B and G
            assert fc(h, A_, k, ptr(W), n, ptr(W), n, G_, m, nrhs, None) == -4                                  # in place
            assert fe(h, A_, k, ptr(wg[:half]), n, Tk, m, ptr(wg[half - 1:]), n, nrhs, None) == -4              # X and W
            assert fe(h, A_, k, Wk, n, ptr(wg[:m * nrhs]), m, ptr(wg[m * nrhs - 1:]), n, nrhs, None) == -4      # X and XT
            assert fe(h, A_, k, ptr(W), n, Tk, m, ptr(W), n, nrhs, None) == -4                                  # in place
            if ar is c.arena:
                assert fc(h, ptr(big[:na]), k, B_, n, ptr(big[na - 1:]), n, G_, m, nrhs, None) == -4           # W and the arena
                assert fe(h, ptr(big[:na]), k, Wk, n, Tk, m, ptr(big[na - 1:]), n, nrhs, None) == -4           # X and the arena
            assert fc(part.h, A_, k, B_, n, W_, n, G_, m, nrhs, None) == -4 and fe(part.h, A_, k, Wk, n, Tk, m, X_, n, nrhs, None) == -4
            assert "partitioned" in L.cholamd_last_error().decode()
    dev.sync()
    for t in (wb, gb, xb, big, wg):
        assert bool((t == SENT).all()), "a refused call wrote something"
    assert torch.equal(c.arena, snap)
    # the Python layer's own checks
    with pytest.raises(ValueError):
        dev.schur_condense_nrhs(c.arena, k, Bv, W=torch.empty((nrhs + 1, n), dtype=torch.float64, device="cuda").T)
    with pytest.raises(ValueError):
        dev.schur_condense_nrhs(c.arena, k, torch.empty((n, nrhs), dtype=torch.float64, device="cuda"))        # row-major
    with pytest.raises(ValueError):
        dev.schur_expand_nrhs(c.arena, k, W_ok, torch.empty((nrhs, m + 1), dtype=torch.float64, device="cuda").T)
    with pytest.raises(ca.CholamdError):
        dev.set_option("schur_deterministic_block", 1)


def test_the_switch_goes_back(ctx, monkeypatch):
    """Off, on, off: the off results agree to rounding, no gather launch runs with the option off; the environment variable sets it at creation."""
    import torch
    import cholesky_amd as ca
    c = ctx("lapl_3375x3375", 2)
    dev = c.dev
    fixed_xt(c)
    runs, counts = [], []
    for det in (0, 1, 0):
        dev.set_option("schur_deterministic", det)
        before = dev.schur_launches()
        runs.append(det_outputs(c, dev, False) + det_outputs(c, dev, True))
        after = dev.schur_launches()
        counts.append({key: after[key] - before[key] for key in after})
    print(f"launches off / on / off: {counts}")
    for off in (counts[0], counts[2]):
        assert off["gather"] == 0 and off["span"] == 0 and off["atomic"] > 0 and off["copy"] > 0
    assert counts[1]["atomic"] == 0 and counts[1]["gather"] > 0 and counts[1]["span"] > 0 and counts[1]["copy"] > 0
    assert counts[0] == counts[2]
    for p, q, r in zip(runs[0], runs[2], runs[1]):
        scale = float(p.abs().max())
        e_off, e_on = float((p - q).abs().max()) / scale, float((p - r).abs().max()) / scale
        print(f"off vs off {e_off:.3g}, off vs on {e_on:.3g}")
        assert e_off <= 1e-12 and e_on <= 1e-12
    monkeypatch.setenv("CHOLAMD_SCHUR_DETERMINISTIC", "1")
    dev_env = ca.Device(c.plan, 0)
    monkeypatch.delenv("CHOLAMD_SCHUR_DETERMINISTIC")
    outs = det_outputs(c, dev_env, False)
    got = dev_env.schur_launches()
    assert got["gather"] > 0 and got["atomic"] == 0
    for p, q in zip(runs[1][:6], outs):
        assert torch.equal(p, q), "the environment's device object returns the option's bits"
    dev_env.set_option("schur_deterministic", 0)                     # ... and set_option takes it back
    det_outputs(c, dev_env, False)
    assert dev_env.schur_launches()["gather"] == got["gather"]
