"""The deterministic BLOCK solve on the device (device options solve_deterministic + solve_deterministic_block): cholamd_solve_nrhs / _f32,
cholamd_solve_half_nrhs / _f32 and cholamd_solve_refine_nrhs on chunks of 32 columns with every off-diagonal contribution gathered by the owner of its
target on 16 x 32 MFMA tiles (k_solve_det_gather_nrhs of chol_solve_det.hip) and the spans solved by the block solve's span kernel in its substitution
form -- the same bits from call to call, and every column's bits independent of the other columns.  Every test sets BOTH options before its first solve
(Input.factored), so none passes without the feature: a library without it refuses the option's name.

Inputs, the smallest at which the lists or the kernel can go wrong:
  tree_tiny               separators of 1 to 33 columns: items of fewer than 16 positions
  tree_single             one separator of 300 columns: two spans, in-block sources only
  tree_over, tree_at      257 / 273 and 256 / 272 columns, either side of the 256-column span boundary, a band-17 leaf
  gen_23_529              Problem(23, 23, 23, 4, 32): a root of 529 columns, three spans; sources longer than 128 steps: every wave has several chunks
  lapl_3375x3375          the fixture
  g7_ragged               a general SPD input with mixed signs (spd_inputs)
Column counts: 1, 5 (a partial chunk, the first half of the tile), 20 (into the second half), 32 (a full chunk), 33 (a second chunk of one column) and 40
at a leading dimension of n + 3.  B: column 0 is the input's own b, the others are seeded normal columns scaled by the input's equilibration.

Gates -- none is measured from the code under test:
  * bits: torch.equal between two calls, a second device object, a device object with poisoned buffers, in place, BACKWARD(FORWARD(B)) and the solve;
    between a column inside a block, the same column at another position, beside a NaN column, and alone.
  * accuracy, per column, the gates of tests/test_gpu_solve_det.py: the SPD inputs and the trees at backward_error <= tol_backward(u) and forward_error <=
    tol_forward(u), u = 2^-53 / 2^-24 by the factor, against a dense numpy solve of the input's matrix with one long-double correction (column 0: the
    input's x_ref); the Laplacians at 1e-9 scale (fp64) / 1e-3 scale (fp32) against the CPU oracle's solve of column 0 and of the last column.  The
    difference to the column-wise deterministic solve (solve_deterministic_block = 0 on the same device object) within twice the gate, in that file's
    measures (the triangle inequality of two solutions that each meet it).
  * refinement, run twice on 5 and on 33 columns: the same corrections, relres and bits; the gates of test_refinement_repeats_itself (the Laplacians: rel <=
    1e-12, at most 8 corrections, 1e-10 scale against the oracle; the others: rel <= 1e-12 within SPD.refine_iterations, forward_error <= tol_forward())."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tree_inputs  # noqa: E402
from conftest import case_paths  # noqa: E402
from guarded import Guarded  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from spd_inputs import U32, U64  # noqa: E402
from test_gpu_general_spd import MAX_ITER  # noqa: E402

FWD, BWD, BOTH = 0, 1, -1
PRECISIONS = [False, True]
PIDS = ["fp64", "fp32"]
GRIDS = {"gen_23_529": (23, 23, 23, 4, 32)}
LAPL = list(GRIDS) + ["lapl_3375x3375"]
NAMES = ["tree_tiny", "tree_single", "tree_over", "tree_at"] + LAPL + ["g7_ragged"]
KMAX = 40
COUNTS = [(1, 0), (5, 0), (20, 0), (32, 0), (33, 0), (40, 3)]   # (columns, ld - n)
SENTINEL = -7.25


@pytest.fixture(autouse=True)
def environment(monkeypatch):
    for v in ("CHOLAMD_POISON", "CHOLAMD_SOLVE_NO_BAND", "CHOLAMD_SOLVE_NO_INV256", "CHOLAMD_SOLVE_REFERENCE_SHAPE", "CHOLAMD_SOLVE_DETERMINISTIC",
              "CHOLAMD_SOLVE_DETERMINISTIC_BLOCK"):
        monkeypatch.delenv(v, raising=False)


class Input:
    """plan, B (n x KMAX), the reference columns (xref[j]: every column of the SPD inputs and trees, columns 0 and KMAX - 1 of the Laplacians) and the
    factored arenas of one input; built once per module."""

    def __init__(self, name, factory):
        import cholesky_amd as ca
        self.name, self.S = name, None
        rng = np.random.default_rng(4242)
        if name in LAPL:
            orc.use_own_kernels()
            if name in GRIDS:
                prob = ca.Problem(*GRIDS[name])
                m, o, c, _ = prob.write(os.path.join(factory.mktemp("sdetn"), "gen"))
                b = prob.rhs()
            else:
                m, o, c, bf = case_paths(name)
                b = ca.plan.read_vector(bf, 3375)
            self.plan = ca.Plan(m, o, c)
            self.B = rng.standard_normal((self.plan.n, KMAX))
            self.B[:, 0] = b
            O = orc.Oracle(m, o, c)
            O.factor()
            self.xref = {j: O.solve(np.ascontiguousarray(self.B[:, j])) for j in (0, KMAX - 1)}
        else:
            S = self.S = tree_inputs.cached(factory, name)
            self.plan = S.plan
            self.B = S.s[:, None] * rng.standard_normal((S.n, KMAX))
            self.B[:, 0] = S.rhs
            A = np.asarray(S.A, dtype=np.float64)
            X = np.linalg.solve(A, self.B)
            R = (self.B.astype(np.longdouble) - A.astype(np.longdouble) @ X.astype(np.longdouble)).astype(np.float64)
            X = X + np.linalg.solve(A, R)
            self.xref = {j: X[:, j] for j in range(KMAX)}
            self.xref[0] = S.x_ref
        self.n = self.plan.n
        self.B.setflags(write=False)
        self.fact = {}

    def factored(self, f32):
        """(device object with BOTH options ON and solve_reference_shape off, arena), factored once per precision."""
        import cholesky_amd as ca
        if f32 not in self.fact:
            dev = ca.Device(self.plan, 0)
            a = dev.new_arena_f32() if f32 else dev.new_arena()
            (dev.fill_f32 if f32 else dev.fill)(a)
            (dev.factor_f32 if f32 else dev.factor)(a)
            dev.sync()
            assert dev.info() == (0, 0)
            self.fact[f32] = (dev, a)
        dev, a = self.fact[f32]
        switch_on(dev)
        return dev, a


def switch_on(dev):
    dev.set_option("solve_reference_shape", 0)
    dev.set_option("solve_deterministic", 1)
    dev.set_option("solve_deterministic_block", 1)


_INPUTS = {}


@pytest.fixture
def inputs(tmp_path_factory):
    def get(name):
        if name not in _INPUTS:
            _INPUTS[name] = Input(name, tmp_path_factory)
        return _INPUTS[name]
    return get


def block(B, pad=0, fill=None):
    """B (numpy, n x k) as a column-major device block at leading dimension n + pad; fill: every element starts as this value instead (an output)."""
    import torch
    n, k = B.shape
    buf = torch.full((k, n + pad), float("nan") if fill is None else fill, dtype=torch.float64, device="cuda")
    t = buf[:, :n].T
    if fill is None:
        t.copy_(torch.from_numpy(np.array(B, dtype=np.float64, order="C")).cuda())
    return t


def run(dev, a, Bt, which, pad=0):
    """solve_nrhs (which = BOTH) or solve_half_nrhs of the device block Bt into a NaN-filled block."""
    Xt = block(np.empty(tuple(Bt.shape)), pad, fill=float("nan"))
    if which == BOTH:
        dev.solve_nrhs(a, Bt, Xt)
    else:
        dev.solve_half_nrhs(a, Bt, Xt, which)
    dev.sync()
    return Xt


def three(dev, a, B, pad):
    Bt = block(B, pad)
    return [run(dev, a, Bt, w, pad) for w in (BOTH, FWD, BWD)]


# ------------------------------------------------------------------------------------------------
# 1., 3.  (a) the same bits, (c) the halves compose
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("name", NAMES)
def test_same_bits(name, f32, inputs, monkeypatch):
    import cholesky_amd as ca
    import torch
    I = inputs(name)
    dev, a = I.factored(f32)                                            # sets the options
    dev2 = ca.Device(I.plan, 0)                                         # another device object, the same plan and arena
    switch_on(dev2)
    monkeypatch.setenv("CHOLAMD_POISON", "1")                           # read at every allocation of the library: this object's buffers start as NaN
    dev3 = ca.Device(I.plan, 0)
    switch_on(dev3)
    for k, pad in COUNTS:
        B = I.B[:, :k]
        first, second = three(dev, a, B, pad), three(dev, a, B, pad)
        for p, q in zip(first, second):
            assert p.shape == (I.n, k) and torch.isfinite(p).all() and torch.equal(p, q), (k, "two calls return other bits")
        for p, q in zip(first, three(dev2, a, B, pad)):
            assert torch.equal(p, q), (k, "a second device object returns other bits")
        for p, q in zip(first, three(dev3, a, B, pad)):
            assert torch.isfinite(q).all() and torch.equal(p, q), (k, "poisoned buffers change the bits")
        # (c) BACKWARD of FORWARD is the solve
        assert torch.equal(run(dev, a, first[1], BWD, pad), first[0]), (k, "BACKWARD(FORWARD(B)) differs from the solve")
        # in place: X == B, ldx == ldb
        for i, which in enumerate((BOTH, FWD, BWD)):
            t = block(B, pad)
            if which == BOTH:
                dev.solve_nrhs(a, t, t)
            else:
                dev.solve_half_nrhs(a, t, t, which)
            dev.sync()
            assert torch.equal(t, first[i]), (k, which, "in place: other bits")
    monkeypatch.delenv("CHOLAMD_POISON")


# ------------------------------------------------------------------------------------------------
# 2.  (b) column independence
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("name", NAMES)
def test_columns_are_independent(name, f32, inputs):
    import torch
    I = inputs(name)
    dev, a = I.factored(f32)                                            # sets the options
    order = np.roll(np.arange(KMAX), 13)                                # column j goes to position (j + 13) mod 40: chunks and halves of the tile change
    Bn = I.B.copy()
    Bn[:, 7] = np.nan
    Bn[3, 35] = np.nan
    keep = [j for j in range(KMAX) if j not in (7, 35)]
    for which in (BOTH, FWD, BWD):
        X = run(dev, a, block(I.B), which)
        assert torch.isfinite(X).all()
        Xp = run(dev, a, block(I.B[:, order]), which)
        assert torch.equal(Xp, X[:, order]), (which, "a column's bits depend on its position")
        Xn = run(dev, a, block(Bn), which)
        assert torch.isnan(Xn[:, 7]).any() and torch.isnan(Xn[:, 35]).any()
        assert torch.equal(Xn[:, keep], X[:, keep]), (which, "a NaN column reached another column")
        for j in range(KMAX):
            x = run(dev, a, block(I.B[:, j:j + 1]), which)
            assert torch.equal(x[:, 0], X[:, j]), (which, j, "a column alone (nrhs = 1) has other bits")


# ------------------------------------------------------------------------------------------------
# 4.  (e) caller memory
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("name", ["tree_tiny", "tree_over", "lapl_3375x3375"])
def test_caller_memory_is_respected(name, f32, inputs):
    import torch
    I = inputs(name)
    dev, a = I.factored(f32)                                            # sets the options
    n = I.n
    for k, pad in ((5, 3), (33, 3), (40, 0)):
        Bg = Guarded(n, k, n + pad, values=I.B[:, :k].copy())
        snap = Bg.snapshot()
        for which in (BOTH, FWD, BWD):
            want = run(dev, a, Bg.t, which)
            Xg = Guarded(n, k, n + pad)                                 # guards and padding rows: a fixed NaN pattern
            wide = torch.full((k + 2, n + pad), SENTINEL, dtype=torch.float64, device="cuda")   # two columns past nrhs
            for X in (Xg.t, wide[:k, :n].T):
                if which == BOTH:
                    dev.solve_nrhs(a, Bg.t, X)
                else:
                    dev.solve_half_nrhs(a, Bg.t, X, which)
                dev.sync()
                assert torch.equal(X, want)
            Xg.assert_guards(f"{name} k={k} which={which}")
            Bg.assert_unchanged(snap, f"{name} k={k} which={which}: B")
            assert (wide[k:, :] == SENTINEL).all(), "columns past nrhs were written"
            assert (wide[:, n:] == SENTINEL).all(), "rows n .. ld - 1 were written"


# ------------------------------------------------------------------------------------------------
# 5.  accuracy
# ------------------------------------------------------------------------------------------------
def check_column(I, j, x, xc, b, f32, tag):
    """Column j of the block solve (x) at the single deterministic solve's gate; its difference to the column-wise deterministic solve (xc) within twice it."""
    u = U32 if f32 else U64
    assert np.isfinite(x).all(), tag
    if I.S is None:
        gate = (1e-3 if f32 else 1e-9) * max(1.0, float(np.abs(xc).max()))   # (the column's own scale, from the column-wise solve it is compared with)
        d = float(np.abs(x - xc).max())
        assert d <= 2 * gate, (tag, d, 2 * gate)
        if j in I.xref:
            gate_j = (1e-3 if f32 else 1e-9) * max(1.0, float(np.abs(I.xref[j]).max()))
            e = float(np.abs(x - I.xref[j]).max())
            print(f"{tag}: |x - x_oracle| = {e:.3e} (gate {gate_j:.3e}), |x - x_columnwise| = {d:.3e} (gate {2 * gate:.3e})")
            assert e <= gate_j, (tag, e, gate_j)
        return
    S = I.S
    be, fe = S.backward_error(x, b), S.forward_error(x, I.xref[j])
    diff = float((np.abs(S.A @ (x - xc)) / (np.abs(S.A) @ np.abs(x) + np.abs(b))).max())
    print(f"{tag}: backward error {be:.3e} (tol {S.tol_backward(u):.3e}), forward error {fe:.3e} (tol {S.tol_forward(u):.3e}), "
          f"difference to the column-wise solve {diff:.3e} (gate {2 * S.tol_backward(u):.3e})")
    assert be <= S.tol_backward(u) and fe <= S.tol_forward(u) and diff <= 2 * S.tol_backward(u), tag


@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("name", NAMES)
def test_accuracy(name, f32, inputs):
    I = inputs(name)
    dev, a = I.factored(f32)                                            # sets the options
    Bt = block(I.B, 3)
    X = run(dev, a, Bt, BOTH, 3).cpu().numpy()
    dev.set_option("solve_deterministic_block", 0)                      # the column-wise deterministic solve on the same device object
    Xc = run(dev, a, Bt, BOTH, 3).cpu().numpy()
    dev.set_option("solve_deterministic_block", 1)
    for j in range(KMAX):
        check_column(I, j, X[:, j], Xc[:, j], I.B[:, j], f32, f"{name} {PIDS[f32]} column {j}")


# ------------------------------------------------------------------------------------------------
# 6.  (d) the refinement repeats itself
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 33])
@pytest.mark.parametrize("name", NAMES)
def test_refinement_repeats_itself(name, k, inputs):
    import torch
    I = inputs(name)
    dev, a32 = I.factored(True)                                         # sets the options
    lapl = I.S is None
    tol, max_iter = (1e-13, 20) if lapl else (1e-12, MAX_ITER)           # as tests/test_gpu_solve_det.py's test_refinement_repeats_itself asks for them
    Bt = block(I.B[:, :k])
    runs = []
    for _ in range(2):
        X = block(np.empty((I.n, k)), fill=float("nan"))
        it, rel = dev.solve_refine_nrhs(a32, Bt, X, max_iter=max_iter, tol=tol)
        dev.sync()
        runs.append((it, np.array(rel, copy=True), X))
    (it, rel, X), (it2, rel2, X2) = runs
    print(f"{name} k={k}: {it} corrections, largest relres {rel.max():.3e}")
    assert it == it2 and np.array_equal(rel, rel2) and torch.equal(X, X2)
    X = X.cpu().numpy()
    assert np.isfinite(X).all() and len(rel) == k
    if lapl:
        assert rel.max() <= 1e-12 and it <= 8, (it, rel)
        assert np.abs(X[:, 0] - I.xref[0]).max() <= 1e-10 * max(1.0, float(np.abs(I.xref[0]).max()))
    else:
        assert rel.max() <= 1e-12 and it <= I.S.refine_iterations(1e-12), (it, rel, I.S.refine_iterations(1e-12))
        for j in range(k):
            assert I.S.forward_error(X[:, j], I.xref[j]) <= I.S.tol_forward(), j


# ------------------------------------------------------------------------------------------------
# 7.  the switches go back
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("name", ["tree_over", "lapl_3375x3375"])
def test_the_switches_go_back(name, f32, inputs):
    import torch
    I = inputs(name)
    dev, a = I.factored(f32)                                            # sets the options
    k = 5
    B = I.B[:, :k]
    Bt = block(B)
    blockwise = run(dev, a, Bt, BOTH)
    assert torch.isfinite(blockwise).all()
    try:
        # the block option off: column j has the bits of the single deterministic solve of column j, as before the option existed
        dev.set_option("solve_deterministic_block", 0)
        X = run(dev, a, Bt, BOTH)
        for j in range(k):
            x = torch.full((I.n,), float("nan"), dtype=torch.float64, device="cuda")
            (dev.solve_f32 if f32 else dev.solve)(a, Bt[:, j].contiguous(), x)
            dev.sync()
            assert torch.isfinite(x).all() and torch.equal(X[:, j], x), j
        # solve_deterministic off, the block option still on: no effect -- the atomic block path at its gate
        dev.set_option("solve_deterministic", 0)
        dev.set_option("solve_deterministic_block", 1)
        Xa = run(dev, a, Bt, BOTH).cpu().numpy()
        if I.S is None:
            assert np.abs(Xa[:, 0] - I.xref[0]).max() <= (1e-3 if f32 else 1e-9) * max(1.0, float(np.abs(I.xref[0]).max()))
        else:
            for j in range(k):
                assert I.S.forward_error(Xa[:, j], I.xref[j]) <= I.S.tol_forward(U32 if f32 else U64), j
        # solve_reference_shape wins (fp64 factor): bit for bit what that option alone returns
        if not f32:
            outs = []
            for det in (1, 0):
                dev.set_option("solve_deterministic", det)
                dev.set_option("solve_deterministic_block", det)
                dev.set_option("solve_reference_shape", 1)
                outs.append([run(dev, a, Bt, w) for w in (BOTH, FWD, BWD)])
            for p, q in zip(*outs):
                assert torch.isfinite(p).all() and torch.equal(p, q)
    finally:
        dev.set_option("solve_reference_shape", 0)
    switch_on(dev)
    assert torch.equal(run(dev, a, Bt, BOTH), blockwise), "the block path after the switches went back and forth"


def test_the_environment_sets_the_option(inputs, monkeypatch):
    """CHOLAMD_SOLVE_DETERMINISTIC_BLOCK is read at device creation, as CHOLAMD_SOLVE_DETERMINISTIC is: a device object created under both returns the block
    path's bits without a set_option call."""
    import cholesky_amd as ca
    import torch
    I = inputs("tree_over")
    dev, a = I.factored(False)                                          # sets the options
    Bt = block(I.B[:, :5])
    want = run(dev, a, Bt, BOTH)
    monkeypatch.setenv("CHOLAMD_SOLVE_DETERMINISTIC", "1")
    monkeypatch.setenv("CHOLAMD_SOLVE_DETERMINISTIC_BLOCK", "1")
    dev2 = ca.Device(I.plan, 0)
    got = run(dev2, a, Bt, BOTH)
    dev.set_option("solve_deterministic_block", 0)
    colwise = run(dev, a, Bt, BOTH)
    dev.set_option("solve_deterministic_block", 1)
    assert torch.equal(got, want)
    print(f"block and column-wise results differ in {(want != colwise).sum().item()} of {want.numel()} elements")
