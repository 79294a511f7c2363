"""The device API on a caller's stream.

Every device entry point of include/cholamd.h ends in `void *stream`, and every other GPU test passes none: all of them run on the null stream, where every
launch, blocking copy and clearing is ordered whatever stream argument the library passes on.  torch's pool streams (torch.cuda.Stream()) are non-blocking:
they do not wait for the null stream, so on them a launch that went to the wrong stream, or a lazy upload or clearing that is not ordered before the first
kernel that reads it, is not covered up.  Every test here uses ONE stream at a time; nothing waits on a value, nothing holds a stream open, no graph is
replayed.

a. test_same_result_on_a_callers_stream / test_atomic_solves_on_a_callers_stream: a family of calls on a fresh device object with everything -- tensor
   allocation, lazy uploads and clearing of the first call, the calls themselves -- on s = torch.cuda.Stream(), synchronised only through s, against the same
   sequence on a second fresh object on the null stream.  Bit for bit where include/cholamd.h promises fixed bits; the families that add with atomics are
   held to the gates of their own files (TOL_RESID of test_gpu_factor, 1e-12 within 8 corrections and TOL_X of test_gpu_mixed) with the residual taken on
   the host from the plan's fill.  Outputs start as the guards' NaN pattern, inputs must come back unchanged, guards intact (tests/guarded.py).
b. test_warm_call_only_enqueues: every call the header documents as asynchronous, warm, inside a stream capture on s that is never replayed.  A launch that
   went to another stream runs for real and writes an output; a hidden synchronisation, allocation or blocking copy makes the runtime refuse the capture,
   which the library reports as an error naming the HIP call.  The outputs must still hold the NaN pattern, the inputs their snapshots.  The device object
   is destroyed afterwards: its host-side counters (prog_epoch, info_parity, step_gen, epoch, done_total) have advanced for launches that never ran.
c. test_autograd_follows_the_current_stream: cholesky_amd.autograd under torch.cuda.stream(s); a spy on the Device methods it calls sees the stream of
   every call, the backward pass included, and the results equal those of a run on the default stream bit for bit.

Inputs: lapl_25x25 (n = 25: one residual workgroup, every separator under one span), lapl_400x400 (five levels: Schur at k = 2 and the program launch),
tree_over (pivots of 257 and 273 columns: the big-pivot kernels, the 256-column span inverses and the step launches with their flags; "tiles" couplings).
Blocks have 33 columns (a chunk of 32 and a ragged one) and ld = n + 3.  tests/test_stream_args_host.py reads the stream arguments in the sources."""
import contextlib
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import lowrank_ref as lr  # noqa: E402
import tree_inputs as ti  # noqa: E402
from guarded import Guarded  # noqa: E402
from test_gpu_buffers import destroy  # noqa: E402
from test_gpu_factor import TOL_RESID  # noqa: E402
from test_gpu_mixed import TOL_X  # noqa: E402

NRHS = 33
REFINE_TOL, REFINE_REL, REFINE_MAX_CORRECTIONS = 1e-13, 1e-12, 8     # tests/test_gpu_mixed.py: solve_refine(max_iter=20, tol=1e-13) -> rel <= 1e-12, iters <= 8
F32_SOLVE_REL = 1e-3                                                 # tests/test_gpu_mixed.py: one solve with the fp32 factor alone
DET = {"solve_deterministic": 1}
DET_BLOCK = {"solve_deterministic": 1, "solve_deterministic_block": 1}
SCHUR_K = 2


@pytest.fixture(autouse=True)
def plain_allocations(monkeypatch):
    """CHOLAMD_POISON synchronises the device after every allocation; these tests want the allocations as a user gets them."""
    monkeypatch.delenv("CHOLAMD_POISON", raising=False)


@pytest.fixture(scope="module")
def spd(tmp_path_factory):
    return lambda name: ti.cached(tmp_path_factory, name)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


class Run:
    """A fresh device object of S.plan with `opts` set, and the stream every call of a family gets: a torch stream, its integer handle (the other branch of
    cholesky_amd.device._stream_ptr) or None."""

    def __init__(self, S, stream, opts=None, as_int=False):
        import cholesky_amd as ca
        self.S, self.stream = S, stream
        self.st = None if stream is None else stream.cuda_stream if as_int else stream
        self.dev = ca.Device(S.plan, 0)
        for k, v in (opts or {}).items():
            self.dev.set_option(k, v)

    def on(self):
        """Everything inside runs with the stream as torch's current one (allocations, fills, copies to the host)."""
        import torch
        return torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()

    def sync(self):
        self.dev.sync(self.st)

    def close(self):
        destroy(self.dev)


def values_of(S, scale=1.0):
    """The value array of S in the order of plan.entries()."""
    row, col = S.plan.entries()
    return np.ascontiguousarray(S.A[row, col]) * scale


def rhs_block(S, k=NRHS, seed=5):
    B = S.s[:, None] * np.random.default_rng(seed).standard_normal((S.n, k))
    B[:, 0] = S.rhs
    return B


def block(V):
    return Guarded(V.shape[0], V.shape[1], V.shape[0] + 3, values=V)


def factored(R, f32=False):
    """A guarded arena filled and factored on the run's stream: the first fill and factor of the object when the family starts with it."""
    import torch
    dev = R.dev
    a = Guarded(dev.plan.arena_doubles, dtype=torch.float32 if f32 else torch.float64)
    (dev.fill_f32 if f32 else dev.fill)(a.t, stream=R.st)
    (dev.factor_f32 if f32 else dev.factor)(a.t, stream=R.st)
    R.sync()
    assert dev.info() == (0, 0)                                       # (after the stream has been synchronised, as the header asks)
    a.assert_guards("arena")
    return a


class Checked:
    """Inputs snapshotted, outputs guarded: verify() after the stream has been synchronised."""

    def __init__(self):
        self.ins, self.outs = [], []

    def input(self, g):
        self.ins.append((g, g.snapshot()))
        return g

    def output(self, g):
        self.outs.append(g)
        return g

    def verify(self, what):
        for g, snap in self.ins:
            g.assert_unchanged(snap, f"{what}: an input")
        for g in self.outs:
            g.assert_guards(f"{what}: an output")


# ------------------------------------------------------------------------------------------------
# a. the families: each returns {name: array or scalar}; arrays are compared by their bits
# ------------------------------------------------------------------------------------------------
def fam_factor(R):
    return {"L": factored(R).bits()}


def fam_factor_f32(R):
    return {"L32": factored(R, f32=True).bits()}


def fam_set_values(R):
    S, dev, ck = R.S, R.dev, Checked()
    v = ck.input(Guarded(S.plan.nz, values=values_of(S, 1.5)))       # new values: 1.5 A
    dev.set_values(v.t, check=False, stream=R.st)                    # the first call: uploads the index lists, allocates the status words
    a = Guarded(S.plan.arena_doubles)
    dev.fill(a.t, stream=R.st)
    dev.factor(a.t, stream=R.st)
    status = dev.values_status(stream=R.st)
    R.sync()
    assert dev.info() == (0, 0)
    a.assert_guards("arena")
    ck.verify("set_values")
    assert status == (0, -1, 0, -1)
    return {"L": a.bits(), "status": np.array(status)}


def fam_queries(R):
    S, dev, ck = R.S, R.dev, Checked()
    a = ck.input(factored(R))
    d = ck.output(Guarded(S.n))
    dev.factor_diag(a.t, out=d.t, stream=R.st)
    ld = dev.logdet(a.t, stream=R.st)
    b, x = ck.input(Guarded(S.n, values=S.rhs)), ck.input(Guarded(S.n, values=S.x_ref))
    r = ck.output(Guarded(S.n))
    rel = dev.residual(b.t, x.t, r.t, stream=R.st)                   # the first call: uploads the CSR copy of A
    R.sync()
    ck.verify("queries")
    return {"diag": d.numpy(), "logdet": ld, "relres": rel, "r": r.numpy()}


def fam_multiply(R):
    S, dev, ck = R.S, R.dev, Checked()
    a = ck.input(factored(R))
    z, Z = ck.input(Guarded(S.n, values=S.rhs)), ck.input(block(rhs_block(S)))
    y, yf, yb = (ck.output(Guarded(S.n)) for _ in range(3))
    Y = ck.output(Guarded(S.n, NRHS, S.n + 3))
    dev.multiply(a.t, z.t, y.t, stream=R.st)                         # the first product: uploads the owner lists
    dev.multiply_half(a.t, z.t, yf.t, dev.HALF_FORWARD, stream=R.st)
    dev.multiply_half(a.t, z.t, yb.t, dev.HALF_BACKWARD, stream=R.st)
    dev.multiply_nrhs(a.t, Z.t, Y.t, stream=R.st)
    fr = dev.factor_residual(a.t, z.t, stream=R.st)
    R.sync()
    ck.verify("multiply")
    assert fr <= TOL_RESID
    return {"y": y.numpy(), "yf": yf.numpy(), "yb": yb.numpy(), "Y": Y.numpy(), "factor_residual": fr}


def fam_selinv(R):
    S, dev, ck = R.S, R.dev, Checked()
    a = ck.input(factored(R))
    z, d, e = ck.output(Guarded(S.plan.arena_doubles)), ck.output(Guarded(S.n)), ck.output(Guarded(S.plan.nz))
    dev.selinv(a.t, z.t, stream=R.st)                                # the first call: builds and uploads the gather lists
    dev.selinv_diag(z.t, out=d.t, stream=R.st)
    dev.selinv_entries(z.t, out=e.t, stream=R.st)
    R.sync()
    ck.verify("selinv")
    return {"Z": z.numpy(), "diag": d.numpy(), "entries": e.numpy()}


def fam_values_grad(R):
    S, dev, ck = R.S, R.dev, Checked()
    a = ck.input(factored(R))
    P, Q = ck.input(block(rhs_block(S, seed=6))), ck.input(block(rhs_block(S, seed=7)))
    gp, gl = ck.output(Guarded(S.plan.nz)), ck.output(Guarded(S.plan.nz))
    dev.values_grad_pairs(P.t, Q.t, alpha=-1.0, out=gp.t, stream=R.st)      # the first call: uploads the entry list
    z = Guarded(S.plan.arena_doubles)
    dev.selinv(a.t, z.t, stream=R.st)
    dev.values_grad_logdet(z.t, alpha=0.75, out=gl.t, stream=R.st)
    R.sync()
    ck.verify("values_grad")
    z.assert_guards("Z arena")
    return {"pairs": gp.numpy(), "logdet": gl.numpy()}


def fam_apply(R):
    S, dev, ck = R.S, R.dev, Checked()
    x, X = ck.input(Guarded(S.n, values=S.rhs)), ck.input(block(rhs_block(S)))
    y, Y = ck.output(Guarded(S.n)), ck.output(Guarded(S.n, NRHS, S.n + 3))
    dev.apply(x.t, y.t, stream=R.st)                                 # the first call of the object altogether: uploads the CSR copy of A
    dev.apply_nrhs(X.t, Y.t, stream=R.st)
    R.sync()
    ck.verify("apply")
    assert np.array_equal(bits(y.numpy()), bits(S.plan.apply_host(S.rhs)))       # the header's fma order, bit for bit
    return {"y": y.numpy(), "Y": Y.numpy()}


def fam_det_solves(R):
    """Under solve_deterministic (R's options; with or without solve_deterministic_block)."""
    S, dev, ck = R.S, R.dev, Checked()
    n = S.n
    a, a32 = ck.input(factored(R)), ck.input(factored(R, f32=True))
    b, B = ck.input(Guarded(n, values=S.rhs)), ck.input(block(rhs_block(S)))
    x, x32, xf, xr = (ck.output(Guarded(n)) for _ in range(4))
    X, Xp = ck.output(Guarded(n, NRHS, n + 3)), ck.output(Guarded(n, NRHS, n + 3))
    dev.solve(a.t, b.t, x.t, stream=R.st)                            # the first solve: builds the solve lists, clears the step flags, uploads the step lists
    dev.solve_f32(a32.t, b.t, x32.t, stream=R.st)
    dev.solve_half(a.t, b.t, xf.t, dev.HALF_FORWARD, stream=R.st)
    dev.solve_nrhs(a.t, B.t, X.t, stream=R.st)
    it, rel = dev.solve_refine(a32.t, b.t, xr.t, max_iter=20, tol=REFINE_TOL, stream=R.st)
    its, rels, status = dev.solve_pcg_nrhs(a.t, B.t, Xp.t, max_iter=20, tol=1e-12, stream=R.st)     # the first call: allocates and clears the columns' records
    R.sync()
    ck.verify("deterministic solves")
    return {"x": x.numpy(), "x32": x32.numpy(), "xf": xf.numpy(), "X": X.numpy(), "xr": xr.numpy(), "refine_it": it, "refine_rel": rel,
            "Xp": Xp.numpy(), "pcg_iters": its.copy(), "pcg_relres": rels.copy(), "pcg_status": status.copy()}


def fam_schur(R):
    """Under schur_deterministic."""
    S, dev, ck = R.S, R.dev, Checked()
    n, k, m = S.n, SCHUR_K, S.plan.schur_size(SCHUR_K)
    a = Guarded(S.plan.arena_doubles)
    dev.fill(a.t, stream=R.st)
    dev.schur_factor(a.t, k, stream=R.st)
    R.sync()
    assert dev.info() == (0, 0)
    ck.input(a)
    Sm = ck.output(Guarded(m, m, m + 3))
    dev.schur(a.t, k, out=Sm.t, stream=R.st)                         # the first call with this k: uploads the piece list
    b, B = ck.input(Guarded(n, values=S.rhs)), ck.input(block(rhs_block(S)))
    w, g, x = ck.output(Guarded(n)), ck.output(Guarded(m)), ck.output(Guarded(n))
    W, G, X = ck.output(Guarded(n, NRHS, n + 3)), ck.output(Guarded(m, NRHS, m + 3)), ck.output(Guarded(n, NRHS, n + 3))
    dev.schur_condense(a.t, k, b.t, w.t, g.t, stream=R.st)           # the first call with this k: builds and uploads the cut step lists
    dev.schur_condense_nrhs(a.t, k, B.t, W.t, G.t, stream=R.st)
    R.sync()
    Sh = Sm.numpy()                                                  # the caller's part: S x_T = g on the host, the same bits from the same S and g
    xt, XT = Guarded(m, values=np.linalg.solve(Sh, g.numpy())), block(np.linalg.solve(Sh, G.numpy()))
    ck.input(xt), ck.input(XT)
    dev.schur_expand(a.t, k, w.t, xt.t, x.t, stream=R.st)
    dev.schur_expand_nrhs(a.t, k, W.t, XT.t, X.t, stream=R.st)
    R.sync()
    ck.verify("schur")
    assert S.true_relres(x.numpy(), S.rhs) <= TOL_RESID
    return {"arena": a.bits(), "S": Sh, "w": w.numpy(), "g": g.numpy(), "x": x.numpy(), "W": W.numpy(), "G": G.numpy(), "X": X.numpy()}


def lowrank_block(low, R):
    """LowRank.block() with the copy on the run's stream (block() itself synchronises the device without one)."""
    p, ld = C.c_void_p(), C.c_int64(0)
    assert low.L.cholamd_lowrank_block(low.h, C.byref(p), C.byref(ld)) == 0
    n, k = R.S.n, low.state()[0]
    return R.dev.download(p.value, ld.value * k, stream=R.st).reshape(k, ld.value)[:, :n].T.copy()


def fam_lowrank(R):
    """Under both deterministic solve options: include/cholamd.h promises the bits of W and L_C then, and those of the corrected solves every time."""
    import cholesky_amd as ca
    S, dev, ck = R.S, R.dev, Checked()
    n, k = S.n, 17
    a = ck.input(factored(R))
    U = ck.input(block(lr.build_u(S, k, lr.UPDATE)))
    b, B = ck.input(Guarded(n, values=S.rhs)), ck.input(block(rhs_block(S)))
    x, X = ck.output(Guarded(n)), ck.output(Guarded(n, NRHS, n + 3))
    low = ca.LowRank(dev, k)
    low.set(a.t, U.t, lr.UPDATE, stream=R.st)
    assert low.state() == (k, lr.UPDATE, 0)
    low.solve(a.t, b.t, x.t, stream=R.st)
    low.solve_nrhs(a.t, B.t, X.t, stream=R.st)
    R.sync()
    ck.verify("lowrank")
    out = {"W": lowrank_block(low, R), "LC": low.factor(), "logdet_c": low.logdet_c(), "x": x.numpy(), "X": X.numpy()}
    low.close()
    return out


def same_bits(got, ref, what):
    assert got.keys() == ref.keys()
    for k in got:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.shape == r.shape and g.size > 0, (what, k)
        same = np.array_equal(g, r) if g.dtype.kind in "iub" else np.array_equal(bits(g), bits(r))
        assert same, f"{what}: {k} differs between the caller's stream and the null stream ({int((bits(g.astype(np.float64)) != bits(r.astype(np.float64))).sum())} of {g.size} elements)"
        if g.dtype.kind == "f":
            assert not np.isnan(g).any(), (what, k)                   # (an output that kept its NaN pattern was never written)


def both_runs(family, S, opts, as_int=False):
    """family on a caller's stream, then on the null stream, each on a fresh device object."""
    import torch
    out = []
    for stream in (torch.cuda.Stream(), None):
        R = Run(S, stream, opts, as_int)
        with R.on():
            out.append(family(R))
        R.close()
    return out


FIXED_BITS = [
    # (family, input, device options)
    (fam_factor, "tree_over", {}), (fam_factor, "lapl_400x400", {}), (fam_factor, "lapl_25x25", {}),
    (fam_factor, "tree_over", {"program": 0}), (fam_factor, "lapl_400x400", {"program": 0}),
    (fam_factor_f32, "tree_over", {}), (fam_factor_f32, "lapl_400x400", {}),
    (fam_set_values, "tree_over", {}), (fam_set_values, "lapl_400x400", {}),
    (fam_queries, "tree_over", {}), (fam_queries, "lapl_25x25", {}),
    (fam_multiply, "tree_over", {}), (fam_multiply, "lapl_25x25", {}),
    (fam_selinv, "tree_over", {}), (fam_selinv, "lapl_400x400", {}),
    (fam_values_grad, "tree_over", {}), (fam_values_grad, "lapl_25x25", {}),
    (fam_apply, "tree_over", {}), (fam_apply, "lapl_25x25", {}),
    (fam_det_solves, "tree_over", DET), (fam_det_solves, "tree_over", DET_BLOCK), (fam_det_solves, "lapl_400x400", DET_BLOCK), (fam_det_solves, "lapl_25x25", DET),
    (fam_schur, "lapl_400x400", {"schur_deterministic": 1}), (fam_schur, "tree_over", {"schur_deterministic": 1}),
    (fam_lowrank, "tree_over", DET_BLOCK), (fam_lowrank, "lapl_400x400", DET_BLOCK),
]


def _id(case):
    fam, name, opts = case
    return "-".join([fam.__name__[4:], name] + [f"{k}{v}" for k, v in opts.items()])


@pytest.mark.parametrize("case", FIXED_BITS, ids=_id)
def test_same_result_on_a_callers_stream(case, spd):
    family, name, opts = case
    got, ref = both_runs(family, spd(name), opts)
    same_bits(got, ref, _id(case))


def test_same_result_with_the_stream_as_an_integer(spd):
    """stream = s.cuda_stream, the raw handle as an int: the other branch of _stream_ptr."""
    for family, opts in ((fam_factor, {}), (fam_det_solves, DET_BLOCK)):
        got, ref = both_runs(family, spd("tree_over"), opts, as_int=True)
        same_bits(got, ref, family.__name__)


# ---- the families that add with atomics --------------------------------------------------------------------------------------------------
_AORIG = {}


def a_from_the_fill(S, name):
    """A in original order, dense fp64, from the plan's own fill (as tests/test_gpu_mixed.py builds it)."""
    if name not in _AORIG:
        plan = S.plan
        A = plan.arena_to_dense(plan.fill_host())
        A = A + np.tril(A, -1).T
        Ao = np.zeros_like(A)
        Ao[np.ix_(plan.perm, plan.perm)] = A
        _AORIG[name] = Ao
    return _AORIG[name]


def host_relres(A, X, B):
    R = B - A @ X
    return float((np.linalg.norm(R, axis=0) / np.linalg.norm(B, axis=0)).max())


def fam_atomic_solves(R):
    S, dev, ck = R.S, R.dev, Checked()
    n = S.n
    a, a32 = ck.input(factored(R)), ck.input(factored(R, f32=True))
    b, B = ck.input(Guarded(n, values=S.rhs)), ck.input(block(rhs_block(S)))
    x, x32, xr = (ck.output(Guarded(n)) for _ in range(3))
    X, Xr = ck.output(Guarded(n, NRHS, n + 3)), ck.output(Guarded(n, NRHS, n + 3))
    dev.solve(a.t, b.t, x.t, stream=R.st)                            # the first solve: builds the solve lists and clears the step launches' flags and scratch
    dev.solve_f32(a32.t, b.t, x32.t, stream=R.st)
    dev.solve_nrhs(a.t, B.t, X.t, stream=R.st)
    it, rel = dev.solve_refine(a32.t, b.t, xr.t, max_iter=20, tol=REFINE_TOL, stream=R.st)
    its, rels = dev.solve_refine_nrhs(a32.t, B.t, Xr.t, max_iter=20, tol=REFINE_TOL, stream=R.st)
    R.sync()
    ck.verify("atomic solves")
    return {"x": x.numpy(), "x32": x32.numpy(), "X": X.numpy(), "xr": xr.numpy(), "Xr": Xr.numpy(), "refine": (it, rel), "refine_nrhs": (its, float(rels.max()))}


@pytest.mark.parametrize("name,as_int", [("tree_over", False), ("tree_over", True), ("lapl_400x400", False), ("lapl_25x25", False)],
                         ids=["tree_over", "tree_over-int", "lapl_400x400", "lapl_25x25"])
def test_atomic_solves_on_a_callers_stream(name, as_int, spd):
    """solve, solve_f32, solve_nrhs, solve_refine and solve_refine_nrhs without the deterministic options: the sums are atomic, so the gates are those of
    tests/test_gpu_factor.py and tests/test_gpu_mixed.py, on the caller's stream and on the null stream alike, and x on the stream agrees with x on the
    null stream at TOL_X.  Once with the stream as its integer handle."""
    S = spd(name)
    got, ref = both_runs(fam_atomic_solves, S, {}, as_int)
    A, b, B = a_from_the_fill(S, name), S.rhs, rhs_block(S)
    for what, o in (("caller's stream", got), ("null stream", ref)):
        res = {"x": host_relres(A, o["x"][:, None], b[:, None]), "X": host_relres(A, o["X"], B), "x32": host_relres(A, o["x32"][:, None], b[:, None]),
               "xr": host_relres(A, o["xr"][:, None], b[:, None]), "Xr": host_relres(A, o["Xr"], B)}
        print(f"{name}, {what}: host ||b - A x|| / ||b||: {res}; refine {o['refine']}, refine_nrhs {o['refine_nrhs']}")
        assert res["x"] <= TOL_RESID and res["X"] <= TOL_RESID, (what, res)
        assert res["x32"] < F32_SOLVE_REL, (what, res)
        for key, host in (("refine", res["xr"]), ("refine_nrhs", res["Xr"])):
            it, rel = o[key]
            assert rel <= REFINE_REL and it <= REFINE_MAX_CORRECTIONS, (what, key, it, rel)
            assert host <= TOL_RESID, (what, key, host)
    for k in ("x", "x32", "X", "xr", "Xr"):
        d = float(np.abs(got[k] - ref[k]).max())
        assert d <= TOL_X * max(1.0, float(np.abs(ref[k]).max())), (k, d)


# ------------------------------------------------------------------------------------------------
# b. a warm asynchronous call only enqueues on the caller's stream
# ------------------------------------------------------------------------------------------------
class Capture:
    """What one captured call needs: call() -> None (raises on a non-zero return), the guarded outputs it would write, the guarded buffers it must not touch,
    and restore() for a call that works in place (its target back to the state the capture starts from)."""

    def __init__(self, call, outs=(), ins=(), restore=None):
        self.call, self.outs, self.ins, self.restore = call, list(outs), list(ins), restore


def reset(g):
    g.buf.view(g.itype).fill_(g.pattern)


def untouched(g):
    return bool((g.bits() == g.pattern).all())


def cap_fill(R, f32=False):
    import torch
    a = Guarded(R.S.plan.arena_doubles, dtype=torch.float32 if f32 else torch.float64)
    fill = R.dev.fill_f32 if f32 else R.dev.fill
    return Capture(lambda: fill(a.t, stream=R.st), outs=[a])


def cap_factor(R, f32=False):
    """The arena holds the filled A when the call starts, eagerly and in the capture: a factorisation that ran would change it."""
    a = factored(R, f32)
    fill, factor = (R.dev.fill_f32, R.dev.factor_f32) if f32 else (R.dev.fill, R.dev.factor)
    fill(a.t, stream=R.st)
    return Capture(lambda: factor(a.t, stream=R.st), ins=[a], restore=lambda: fill(a.t, stream=R.st))


def cap_set_values(R):
    """The scatter list is the library's own: what shows is the fill after it, which is part of the eager round only."""
    v = Guarded(R.S.plan.nz, values=values_of(R.S, 1.5))
    return Capture(lambda: R.dev.set_values(v.t, check=False, stream=R.st), ins=[v])


def _vec_case(fn_of):
    """A call with the factor, the right-hand side b and one output vector x."""
    def make(R, f32=False):
        a, b, x = factored(R, f32), Guarded(R.S.n, values=R.S.rhs), Guarded(R.S.n)
        return Capture(fn_of(R, a, b, x), outs=[x], ins=[a, b])
    return make


def _block_case(fn_of):
    def make(R):
        n = R.S.n
        a, B, X = factored(R), block(rhs_block(R.S)), Guarded(n, NRHS, n + 3)
        return Capture(fn_of(R, a, B, X), outs=[X], ins=[a, B])
    return make


def cap_selinv(R, what):
    S, dev = R.S, R.dev
    a, z = factored(R), Guarded(S.plan.arena_doubles)
    if what == "selinv":
        return Capture(lambda: dev.selinv(a.t, z.t, stream=R.st), outs=[z], ins=[a])
    dev.selinv(a.t, z.t, stream=R.st)
    out = Guarded(S.n if what == "selinv_diag" else S.plan.nz)
    if what == "selinv_diag":
        return Capture(lambda: dev.selinv_diag(z.t, out=out.t, stream=R.st), outs=[out], ins=[z])
    if what == "selinv_entries":
        return Capture(lambda: dev.selinv_entries(z.t, out=out.t, stream=R.st), outs=[out], ins=[z])
    return Capture(lambda: dev.values_grad_logdet(z.t, alpha=0.75, out=out.t, stream=R.st), outs=[out], ins=[z])


def cap_values_grad_pairs(R):
    P, Q, out = block(rhs_block(R.S, seed=6)), block(rhs_block(R.S, seed=7)), Guarded(R.S.plan.nz)
    return Capture(lambda: R.dev.values_grad_pairs(P.t, Q.t, alpha=-1.0, out=out.t, stream=R.st), outs=[out], ins=[P, Q])


def cap_apply(R, nrhs):
    n = R.S.n
    x, y = (block(rhs_block(R.S)), Guarded(n, NRHS, n + 3)) if nrhs else (Guarded(n, values=R.S.rhs), Guarded(n))
    fn = R.dev.apply_nrhs if nrhs else R.dev.apply
    return Capture(lambda: fn(x.t, y.t, stream=R.st), outs=[y], ins=[x])


def cap_schur(R, what):
    S, dev, k = R.S, R.dev, SCHUR_K
    n, m = S.n, S.plan.schur_size(k)
    a = Guarded(S.plan.arena_doubles)
    dev.fill(a.t, stream=R.st)
    if what == "schur_factor":
        return Capture(lambda: dev.schur_factor(a.t, k, stream=R.st), ins=[a], restore=lambda: dev.fill(a.t, stream=R.st))
    dev.schur_factor(a.t, k, stream=R.st)
    b, w, g = Guarded(n, values=S.rhs), Guarded(n), Guarded(m)
    if what == "schur_condense":
        return Capture(lambda: dev.schur_condense(a.t, k, b.t, w.t, g.t, stream=R.st), outs=[w, g], ins=[a, b])
    dev.schur_condense(a.t, k, b.t, w.t, g.t, stream=R.st)
    xt, x = Guarded(m, values=np.ones(m)), Guarded(n)
    return Capture(lambda: dev.schur_expand(a.t, k, w.t, xt.t, x.t, stream=R.st), outs=[x], ins=[a, w, xt])


F, B_ = 0, 1  # HALF_FORWARD, HALF_BACKWARD
CAPTURED = {
    # name: (maker, device options)
    "fill": (cap_fill, {}),
    "factor": (cap_factor, {}),
    "factor_levels": (cap_factor, {"program": 0}),
    "fill_f32": (lambda R: cap_fill(R, True), {}),
    "factor_f32": (lambda R: cap_factor(R, True), {}),
    "set_values": (cap_set_values, {}),
    "solve": (_vec_case(lambda R, a, b, x: lambda: R.dev.solve(a.t, b.t, x.t, stream=R.st)), {}),
    "solve_det": (_vec_case(lambda R, a, b, x: lambda: R.dev.solve(a.t, b.t, x.t, stream=R.st)), DET),
    "solve_f32": (lambda R: _vec_case(lambda R, a, b, x: lambda: R.dev.solve_f32(a.t, b.t, x.t, stream=R.st))(R, True), {}),
    "solve_half": (_vec_case(lambda R, a, b, x: lambda: R.dev.solve_half(a.t, b.t, x.t, B_, stream=R.st)), {}),
    "solve_nrhs": (_block_case(lambda R, a, B, X: lambda: R.dev.solve_nrhs(a.t, B.t, X.t, stream=R.st)), {}),
    "solve_nrhs_det": (_block_case(lambda R, a, B, X: lambda: R.dev.solve_nrhs(a.t, B.t, X.t, stream=R.st)), DET_BLOCK),
    "solve_half_nrhs": (_block_case(lambda R, a, B, X: lambda: R.dev.solve_half_nrhs(a.t, B.t, X.t, F, stream=R.st)), {}),
    "multiply": (_vec_case(lambda R, a, b, x: lambda: R.dev.multiply(a.t, b.t, x.t, stream=R.st)), {}),
    "multiply_half": (_vec_case(lambda R, a, b, x: lambda: R.dev.multiply_half(a.t, b.t, x.t, F, stream=R.st)), {}),
    "multiply_nrhs": (_block_case(lambda R, a, B, X: lambda: R.dev.multiply_nrhs(a.t, B.t, X.t, stream=R.st)), {}),
    "factor_diag": (_vec_case(lambda R, a, b, x: lambda: R.dev.factor_diag(a.t, out=x.t, stream=R.st)), {}),
    "selinv": (lambda R: cap_selinv(R, "selinv"), {}),
    "selinv_diag": (lambda R: cap_selinv(R, "selinv_diag"), {}),
    "selinv_entries": (lambda R: cap_selinv(R, "selinv_entries"), {}),
    "values_grad_pairs": (cap_values_grad_pairs, {}),
    "values_grad_logdet": (lambda R: cap_selinv(R, "values_grad_logdet"), {}),
    "apply": (lambda R: cap_apply(R, False), {}),
    "apply_nrhs": (lambda R: cap_apply(R, True), {}),
    "schur_factor": (lambda R: cap_schur(R, "schur_factor"), {}),
    "schur_condense": (lambda R: cap_schur(R, "schur_condense"), {}),
    "schur_expand": (lambda R: cap_schur(R, "schur_expand"), {}),
}


@pytest.mark.parametrize("name", list(CAPTURED))
def test_warm_call_only_enqueues(name, spd):
    """One call per capture on a fresh object that has run the call eagerly on s once.  The graph is dropped without a launch."""
    import torch
    import cholesky_amd as ca
    maker, opts = CAPTURED[name]
    S = spd("tree_over")
    s = torch.cuda.Stream()
    R = Run(S, s, opts)
    with R.on():
        cap = maker(R)
        cap.call()                                                    # eagerly, on s: whatever the call builds, uploads or clears at first use happens here
        R.sync()
        for g in cap.outs:
            g.assert_guards(f"{name}: an output of the eager call")
            assert not np.isnan(g.numpy()).any(), f"{name}: the eager call left NaN in an output: the check below could not see a write"
        if cap.restore:
            cap.restore()
        for g in cap.outs:
            reset(g)
        R.sync()
        snaps = [g.snapshot() for g in cap.ins]
    lib_error = capture_error = None
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph, stream=s):                       # (the default error mode: global)
            try:
                cap.call()
            except ca.CholamdError as e:
                lib_error = e
    except RuntimeError as e:                                         # the capture was invalidated: ending it fails too
        capture_error = e
    torch.cuda.synchronize()
    del graph                                                         # never launched
    try:
        assert lib_error is None, f"{name} did not return 0 inside a stream capture: {lib_error}"
        assert capture_error is None, f"the capture around {name} could not be ended: {capture_error}"
        for g in cap.outs:
            assert untouched(g), f"{name}: an output was written although the captured call never ran: a launch left the caller's stream"
        for g, snap in zip(cap.ins, snaps):
            g.assert_unchanged(snap, f"{name}: an input or the arena")
    finally:
        R.close()                                                     # the object's counters have advanced for launches that never ran: never used again


# ------------------------------------------------------------------------------------------------
# c. autograd follows torch's current stream
# ------------------------------------------------------------------------------------------------
AUTOGRAD_CALLS = ("set_values", "fill", "factor", "sync", "solve_nrhs", "values_grad_pairs", "logdet", "selinv", "values_grad_logdet")


def spy_on(dev, seen):
    """Every Device method cholesky_amd/autograd.py calls, wrapped on this object: the `stream` it was given is recorded."""
    for name in AUTOGRAD_CALLS:
        inner = getattr(dev, name)

        def wrapped(*args, _inner=inner, _name=name, **kw):
            seen.append((_name, kw["stream"] if "stream" in kw else args[0] if _name == "sync" and args else None))
            return _inner(*args, **kw)
        setattr(dev, name, wrapped)


def autograd_round(S, stream):
    import torch
    import cholesky_amd as ca
    n = S.n
    rng = np.random.default_rng(41)
    Bh, Th, th = S.s[:, None] * rng.standard_normal((n, 3)), S.s[:, None] * rng.standard_normal((n, 3)), S.s * rng.standard_normal(n)
    dev = ca.Device(S.plan, 0)
    for o in DET_BLOCK:
        dev.set_option(o, 1)
    seen = []
    spy_on(dev, seen)
    with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
        values = torch.from_numpy(values_of(S)).cuda().requires_grad_(True)
        B = torch.from_numpy(Bh).cuda().requires_grad_(True)
        b = torch.from_numpy(S.rhs.copy()).cuda().requires_grad_(True)
        T, t = torch.from_numpy(Th).cuda(), torch.from_numpy(th).cuda()
        fac = ca.factorize(dev, values)
        X, x, ld = fac.solve(B), fac.solve(b), fac.logdet()
        loss = (T * X).sum() + (t * x).sum() + 0.75 * ld
        loss.backward()
        (stream if stream is not None else torch.cuda.current_stream()).synchronize()
        out = {k: v.detach().cpu().numpy() for k, v in (("values.grad", values.grad), ("B.grad", B.grad), ("b.grad", b.grad), ("X", X), ("x", x), ("logdet", ld))}
    fac.release()
    del fac, loss, X, x, ld
    for name in AUTOGRAD_CALLS:                                       # (the wrappers hold the object: take them off so that it can go)
        delattr(dev, name)
    destroy(dev)
    return out, seen


@pytest.mark.parametrize("name", ["lapl_400x400", "tree_over"])
def test_autograd_follows_the_current_stream(name, spd):
    import torch
    S = spd(name)
    s = torch.cuda.Stream()
    got, seen = autograd_round(S, s)
    ref, seen0 = autograd_round(S, None)
    called = {c for c, _ in seen}
    assert called == set(AUTOGRAD_CALLS), set(AUTOGRAD_CALLS) - called
    assert {c for c, _ in seen0} == called
    wrong = [(c, st) for c, st in seen if st is None or st.cuda_stream != s.cuda_stream]
    assert not wrong, f"autograd passed another stream than torch's current one: {wrong}"
    assert sum(c == "solve_nrhs" for c, _ in seen) == 4 and sum(c == "values_grad_pairs" for c, _ in seen) == 2       # two solves forward, their two adjoints
    same_bits(got, ref, f"autograd {name}")
