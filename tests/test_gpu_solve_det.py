"""The deterministic streamed solve on the device (device option solve_deterministic): cholamd_solve / _f32, cholamd_solve_half / _f32 and
cholamd_solve_refine with every off-diagonal contribution gathered by the owner of its target (chol_solve_det.hip) -- the same bits from call to
call, for an fp64 and an fp32 factor.  Every test sets the option before its first solve (Input.factored), so none passes without it.

Inputs, the smallest at which the lists or the kernels can go wrong:
  tree_tiny               separators of 1 to 33 columns: chunks of fewer than 16 positions
  tree_single             one separator of 300 columns: two spans, the in-block gather alone
  tree_two                band and arrow leaves
  tree_over, tree_at      257 / 273 and 256 / 272 columns, either side of the span boundary, a band-17 leaf
  gen_18_324              Problem(18, 18, 18, 3, 48): a root of 324 = 256 + 68 columns
  gen_23_529              Problem(23, 23, 23, 4, 32): a root of 529 columns, three spans -- a source two spans back
  lapl_3375x3375          the fixture the one-launch program factors
  g7_ragged, g18_full     general SPD inputs with mixed signs (spd_inputs)

Gates -- none is measured from the code under test:
  * bits: torch.equal between two calls, a second device object, a device object with poisoned buffers, in place, and BACKWARD(FORWARD(b)).
  * the Laplacians against the CPU oracle's x: test_ragged_root_span_solves' gates, 1e-9 scale (fp64 factor) and 1e-3 scale (one fp32-factor solve),
    scale = max(1, |x|_max); against the atomic path on the same device: twice that.
  * the SPD inputs and the trees (spd_inputs' derived bounds, u = 2^-53 / 2^-24 by the factor): backward_error <= tol_backward(u) and forward_error
    <= tol_forward(u); against the atomic path: the backward error of the difference, max |A (x - x')| / (|A| |x| + |b|), within twice tol_backward(u)
    (the triangle inequality of two solutions that each meet it).
  * refinement, run twice: the same corrections, relres and bits of x; the Laplacians at test_ragged_root_span_solves' gates (rel <= 1e-12, at most 8
    corrections, 1e-10 scale against the oracle), the others at test_gpu_trees' (rel <= 1e-12 within SPD.refine_iterations, forward_error <= tol_forward()).
  * multiply_half(w)(solve_half(w)(b)) against b within tol_forward(u) = C_FE (k + 1) u kappa, FORWARD: max |S^-1 (M y - b)| / max |S^-1 b| for a
    right-hand side b, BACKWARD: max |M^T x - b| / max |b| for a white b (the measures of tests/test_solve_det_host.py)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tree_inputs  # noqa: E402
from conftest import case_paths  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from spd_inputs import C_FE, U32, U64  # noqa: E402
from test_gpu_general_spd import MAX_ITER  # noqa: E402

FWD, BWD = 0, 1
PRECISIONS = [False, True]
PIDS = ["fp64", "fp32"]
TREES = ["tree_tiny", "tree_single", "tree_two", "tree_over", "tree_at"]
GRIDS = {"gen_18_324": (18, 18, 18, 3, 48), "gen_23_529": (23, 23, 23, 4, 32)}
SPDS = ["g7_ragged", "g18_full"]
NAMES = TREES + list(GRIDS) + ["lapl_3375x3375"] + SPDS


@pytest.fixture(autouse=True)
def environment(monkeypatch):
    for v in ("CHOLAMD_POISON", "CHOLAMD_SOLVE_NO_BAND", "CHOLAMD_SOLVE_NO_INV256", "CHOLAMD_SOLVE_REFERENCE_SHAPE", "CHOLAMD_SOLVE_DETERMINISTIC"):
        monkeypatch.delenv(v, raising=False)


class Input:
    """plan, b, the reference x (the oracle's for the Laplacians, spd_inputs' for the others) and the factored arenas of one input."""

    def __init__(self, name, factory):
        import cholesky_amd as ca
        self.name, self.S = name, None
        if name in GRIDS or name == "lapl_3375x3375":
            orc.use_own_kernels()
            if name in GRIDS:
                prob = ca.Problem(*GRIDS[name])
                m, o, c, _ = prob.write(os.path.join(factory.mktemp("sdet"), "gen"))
                self.b = prob.rhs()
            else:
                m, o, c, bf = case_paths(name)
                self.b = ca.plan.read_vector(bf, 3375)
            self.plan = ca.Plan(m, o, c)
            O = orc.Oracle(m, o, c)
            O.factor()
            self.x_ref = O.solve(self.b)
        else:
            self.S = tree_inputs.cached(factory, name)
            self.plan, self.b, self.x_ref = self.S.plan, self.S.rhs, self.S.x_ref
        self.n = self.plan.n
        self.scale = max(1.0, float(np.abs(self.x_ref).max()))
        self.fact = {}

    def factored(self, f32):
        """(device object with the option ON, arena), factored once per precision."""
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
        dev.set_option("solve_deterministic", 1)
        return dev, a


_INPUTS = {}


@pytest.fixture
def inputs(tmp_path_factory):
    def get(name):
        if name not in _INPUTS:
            _INPUTS[name] = Input(name, tmp_path_factory)
        return _INPUTS[name]
    return get


def cuda(v):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).cuda()


def nan_vec(n):
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def three(dev, a, b):
    """(solve, FORWARD half, BACKWARD half) of b as device tensors, out of place into NaN-filled vectors."""
    t = cuda(b)
    out = [nan_vec(len(b)) for _ in range(3)]
    (dev.solve_f32 if dev._is_f32(a) else dev.solve)(a, t, out[0])
    dev.solve_half(a, t, out[1], FWD)
    dev.solve_half(a, t, out[2], BWD)
    dev.sync()
    return out


def check_accuracy(I, x, xa, f32, tag):
    """x (deterministic) and xa (atomic path) against the input's gates."""
    u = U32 if f32 else U64
    assert np.isfinite(x).all()
    if I.S is None:
        gate = (1e-3 if f32 else 1e-9) * I.scale
        e, d = float(np.abs(x - I.x_ref).max()), float(np.abs(x - xa).max())
        print(f"{tag}: |x - x_oracle| = {e:.3e} (gate {gate:.3e}), |x - x_atomic| = {d:.3e} (gate {2 * gate:.3e})")
        assert e <= gate and d <= 2 * gate
        return
    S = I.S
    be, fe = S.backward_error(x, S.rhs), S.forward_error(x)
    Al = np.abs(S.A)
    diff = float((np.abs(S.A @ (x - xa)) / (Al @ np.abs(x) + np.abs(S.rhs))).max())
    print(f"{tag}: backward error {be:.3e} (tol {S.tol_backward(u):.3e}), forward error {fe:.3e} (tol {S.tol_forward(u):.3e}), "
          f"difference to the atomic path {diff:.3e} (gate {2 * S.tol_backward(u):.3e})")
    assert be <= S.tol_backward(u) and fe <= S.tol_forward(u) and diff <= 2 * S.tol_backward(u)


# ------------------------------------------------------------------------------------------------
# 1. - 3., 7.  bits, composition, accuracy, and the switch goes back
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("name", NAMES)
def test_same_bits_and_accuracy(name, f32, inputs, monkeypatch):
    import cholesky_amd as ca
    import torch
    I = inputs(name)
    dev, a = I.factored(f32)                                            # sets the option
    first, second = three(dev, a, I.b), three(dev, a, I.b)
    for p, q in zip(first, second):
        assert torch.isfinite(p).all() and torch.equal(p, q), "two calls return other bits"
    dev2 = ca.Device(I.plan, 0)                                         # another device object, the same plan and arena
    dev2.set_option("solve_deterministic", 1)
    for p, q in zip(first, three(dev2, a, I.b)):
        assert torch.equal(p, q), "a second device object returns other bits"
    monkeypatch.setenv("CHOLAMD_POISON", "1")                           # read at every allocation of the library: this object's buffers start as NaN
    dev3 = ca.Device(I.plan, 0)
    dev3.set_option("solve_deterministic", 1)
    for p, q in zip(first, three(dev3, a, I.b)):
        assert torch.isfinite(q).all() and torch.equal(p, q), "poisoned buffers change the bits"
    monkeypatch.delenv("CHOLAMD_POISON")
    # 2. BACKWARD of FORWARD is the solve; in place
    y = nan_vec(I.n)
    dev.solve_half(a, first[1], y, BWD)
    dev.sync()
    assert torch.equal(y, first[0]), "BACKWARD(FORWARD(b)) differs from the solve"
    t = cuda(I.b)
    (dev.solve_f32 if f32 else dev.solve)(a, t, t)
    dev.sync()
    assert torch.equal(t, first[0]), "in place: other bits"
    for which in (FWD, BWD):
        t = cuda(I.b)
        dev.solve_half(a, t, t, which)
        dev.sync()
        assert torch.equal(t, first[1 + which]), "half solve in place: other bits"
    # 7. the option off again: the atomic path, at the existing gate; 3. accuracy of both
    dev.set_option("solve_deterministic", 0)
    xa = nan_vec(I.n)
    (dev.solve_f32 if f32 else dev.solve)(a, cuda(I.b), xa)
    dev.sync()
    xa = xa.cpu().numpy()
    if I.S is None:
        assert np.abs(xa - I.x_ref).max() <= (1e-3 if f32 else 1e-9) * I.scale
    else:
        assert I.S.forward_error(xa) <= I.S.tol_forward(U32 if f32 else U64)
    check_accuracy(I, first[0].cpu().numpy(), xa, f32, f"{name} {PIDS[f32]}")


# ------------------------------------------------------------------------------------------------
# 4. refinement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_refinement_repeats_itself(name, inputs):
    import torch
    I = inputs(name)
    dev, a32 = I.factored(True)                                         # sets the option
    lapl = I.S is None
    tol, max_iter = (1e-13, 20) if lapl else (1e-12, MAX_ITER)           # as test_ragged_root_span_solves / test_gpu_trees ask for them
    runs = []
    for _ in range(2):
        x = nan_vec(I.n)
        it, rel = dev.solve_refine(a32, cuda(I.b), x, max_iter=max_iter, tol=tol)
        dev.sync()
        runs.append((it, rel, x))
    (it, rel, x), (it2, rel2, x2) = runs
    print(f"{name}: {it} corrections, relres {rel:.3e}")
    assert it == it2 and rel == rel2 and torch.equal(x, x2)
    x = x.cpu().numpy()
    if lapl:
        assert rel <= 1e-12 and it <= 8, (it, rel)
        assert np.abs(x - I.x_ref).max() <= 1e-10 * I.scale
    else:
        assert rel <= 1e-12 and it <= I.S.refine_iterations(1e-12), (it, rel, I.S.refine_iterations(1e-12))
        assert I.S.forward_error(x) <= I.S.tol_forward()


# ------------------------------------------------------------------------------------------------
# 5. the product undoes the half solve
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("name", TREES + SPDS)
def test_product_undoes_the_half_solve(name, f32, inputs):
    I = inputs(name)
    dev, a = I.factored(f32)                                            # sets the option
    S = I.S
    tol = C_FE * (S.k + 1) * (U32 if f32 else U64) * S.kappa             # S.tol_forward(u)
    w = np.random.default_rng(41).standard_normal(S.n)
    for which, b in ((FWD, S.s * w), (BWD, w)):
        y = nan_vec(S.n)
        dev.solve_half(a, cuda(b), y, which)
        dev.multiply_half(a, y, y, which)
        dev.sync()
        r = y.cpu().numpy() - b
        e = float(np.abs(r / S.s).max() / np.abs(w).max()) if which == FWD else float(np.abs(r).max() / np.abs(w).max())
        print(f"{name} {PIDS[f32]} which={which}: {e:.3e} (tol {tol:.3e})")
        assert e <= tol


# ------------------------------------------------------------------------------------------------
# 6. the block entry points go column by column
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", PRECISIONS, ids=PIDS)
@pytest.mark.parametrize("name", ["tree_over", "gen_18_324"])
def test_nrhs_is_the_columnwise_solve(name, f32, inputs):
    import torch
    I = inputs(name)
    dev, a = I.factored(f32)                                            # sets the option
    B = np.random.default_rng(42).standard_normal((I.n, 5)) * (I.S.s[:, None] if I.S is not None else 1.0)
    B[:, 0] = I.b
    Bt = torch.from_numpy(np.ascontiguousarray(B.T)).cuda().T           # column-major n x 5
    Xt = torch.full((5, I.n), float("nan"), dtype=torch.float64, device="cuda").T
    dev.solve_nrhs(a, Bt, Xt)
    for which in (FWD, BWD):
        Ht = torch.full((5, I.n), float("nan"), dtype=torch.float64, device="cuda").T
        dev.solve_half_nrhs(a, Bt, Ht, which)
        for j in range(5):
            x = nan_vec(I.n)
            dev.solve_half(a, cuda(B[:, j]), x, which)
            dev.sync()
            assert torch.equal(Ht[:, j], x), (which, j)
    for j in range(5):
        x = nan_vec(I.n)
        (dev.solve_f32 if f32 else dev.solve)(a, cuda(B[:, j]), x)
        dev.sync()
        assert torch.isfinite(x).all() and torch.equal(Xt[:, j], x), j


def test_reference_shape_keeps_precedence(inputs):
    """Both options set on an fp64 factor: the per-call kernels run, bit for bit what solve_reference_shape alone returns."""
    import torch
    I = inputs("tree_over")
    dev, a = I.factored(False)                                          # sets the option
    outs = []
    for det in (1, 0):
        dev.set_option("solve_deterministic", det)
        dev.set_option("solve_reference_shape", 1)
        x = nan_vec(I.n)
        dev.solve(a, cuda(I.b), x)
        dev.sync()
        outs.append(x)
    dev.set_option("solve_reference_shape", 0)
    assert torch.equal(outs[0], outs[1])
