"""Gradients with respect to the value array: the two contraction kernels, a whole backward pass next to the forward block solve, and the same contraction
done with torch indexing (development aid; bench.py is the contract).

python scripts/values_grad_bench.py CASE NRHS [reps]
  CASE = a fixture under tests/golden, gen:NXxNYxNZ:levels:tile or gen:N:levels (an N^3 grid, tile 64); NRHS = columns of B.  fp64 factor.  Everything is
  timed with HIP events on one stream: one warm-up round, then `reps` rounds in which every variant runs ONCE, in turn (interleaved repetitions), each
  between its own pair of events; reported as median [min, max] in ms, beside the mean time of an empty event pair (cholamd_device_event_overhead).
    pairs            cholamd_values_grad_pairs on Lam, X (n x NRHS each)
    logdet           cholamd_values_grad_logdet on the Z arena
    selinv           cholamd_selinv (what the first backward pass of a logdet adds, once per Factorization)
    solve_nrhs       cholamd_solve_nrhs, NRHS columns: the forward pass, and the adjoint solve of the backward pass
    backward         the backward pass of Factorization.solve through torch.autograd: adjoint block solve + pairs (+ torch's copies into column-major blocks)
    torch_index      what a caller had before: -(Lam[i] * X[j] + Lam[j] * X[i]).sum(1) (halved on the diagonal) with index tensors kept on the device
    torch_index_add  the scatter form: index_add_ of the off-diagonal products of both triangles into the value array (not deterministic)
  Derived: pairs over solve_nrhs, and the bytes the pair kernel must move at least (the four row gathers, 4 * 8 * NRHS bytes per entry when nothing is
  reused, the three index arrays and the store) over its time.  The two results are compared (max difference relative to the largest entry).
  Prints one JSON line."""
import json
import os
import statistics
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cholesky_amd as ca  # noqa: E402

case = sys.argv[1] if len(sys.argv) > 1 else "lapl_3375x3375"
nrhs = int(sys.argv[2]) if len(sys.argv) > 2 else 32
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
if case.startswith("gen:"):
    parts = case.split(":")
    dims, lv, tile = parts[1], parts[2], parts[3] if len(parts) > 3 else 64
    nx, ny, nz = (int(v) for v in dims.split("x")) if "x" in dims else (int(dims),) * 3
    plan = ca.Problem(nx, ny, nz, int(lv), int(tile)).plan()
else:
    G = os.path.join(root, "tests", "golden", case)
    files = sorted(os.listdir(G))
    mtx = [f for f in files if f.startswith("lapl") and f.endswith(".mtx")][0]
    plan = ca.Plan(os.path.join(G, mtx), os.path.join(G, [f for f in files if "_ord_" in f][0]), os.path.join(G, [f for f in files if "_clust_" in f][0]))
dev = ca.Device(plan, 0)
n, nzv = plan.n, plan.nz
row_h, col_h = plan.entries()
stream = torch.cuda.current_stream()


def cm(rows, cols):
    t = torch.empty((cols, rows), dtype=torch.float64, device="cuda").T
    t.copy_(torch.rand((rows, cols), dtype=torch.float64, device="cuda") - 0.5)
    return t


# the plan's own values as the value array: the non-zeros of the plan's fill are its scatter list in order (ascending arena offsets), value_map() their
# indices in the value array (a generated problem and the fixtures have no explicit zeros and no duplicates)
host_arena = plan.fill_host()
pos = np.nonzero(host_arena)[0]
vm = plan.value_map()
assert len(pos) == len(vm) == nzv, "the plan has entries outside the pattern: give it a value array of your own"
vals_np = np.zeros(nzv)
vals_np[vm] = host_arena[pos]
values = torch.from_numpy(vals_np).cuda().requires_grad_(True)
fac = ca.factorize(dev, values)
arena = fac.arena
B, T, X, Lam = cm(n, nrhs), cm(n, nrhs), cm(n, nrhs), cm(n, nrhs)
dev.solve_nrhs(arena, B, X)
dev.solve_nrhs(arena, T, Lam)
g = torch.empty(nzv, dtype=torch.float64, device="cuda")
g2 = torch.empty(nzv, dtype=torch.float64, device="cuda")
z = dev.selinv(arena)
ri, ci = torch.from_numpy(row_h).cuda().long(), torch.from_numpy(col_h).cuda().long()
diag = ri == ci
off_r, off_c = ri[~diag], ci[~diag]
k_off = torch.nonzero(~diag).squeeze(1)
k_diag = torch.nonzero(diag).squeeze(1)
Xr, Lr = X.contiguous(), Lam.contiguous()                     # row-major copies: what torch indexing gathers rows from


def torch_index():
    s = (Lr[ri] * Xr[ci]).sum(1) + (Lr[ci] * Xr[ri]).sum(1)
    return -torch.where(diag, 0.5 * s, s)


def torch_index_add():
    out = torch.zeros(nzv, dtype=torch.float64, device="cuda")
    out.index_add_(0, k_off, -(Lr[off_r] * Xr[off_c]).sum(1))
    out.index_add_(0, k_off, -(Lr[off_c] * Xr[off_r]).sum(1))
    out.index_add_(0, k_diag, -(Lr[ri[diag]] * Xr[ri[diag]]).sum(1))
    return out


Bleaf = B.detach().clone().requires_grad_(True)
Xout = fac.solve(Bleaf)


def backward():
    values.grad = None
    Bleaf.grad = None
    Xout.backward(T, retain_graph=True)


variants = {
    "pairs": lambda: dev.values_grad_pairs(Lam, X, alpha=-1.0, out=g),
    "logdet": lambda: dev.values_grad_logdet(z, out=g2),
    "selinv": lambda: dev.selinv(arena, z),
    "solve_nrhs": lambda: dev.solve_nrhs(arena, B, X),
    "backward": backward,
    "torch_index": torch_index,
    "torch_index_add": torch_index_add,
}
times = {name: [] for name in variants}
for rep in range(reps + 1):                            # round 0 warms every variant up
    for name, fn in variants.items():
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        e.record(stream)
        e.synchronize()
        if rep:
            times[name].append(a.elapsed_time(e))


def stats(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


res = dict(case=case, n=n, nz=nzv, nrhs=nrhs, reps=reps, device=torch.cuda.get_device_name(0), event_pair_ms=round(dev.event_overhead_ms(), 4))
for name, v in times.items():
    res[name + "_ms"] = stats(v)
med = lambda key: res[key + "_ms"]["median"]  # noqa: E731
res["pairs_over_solve_nrhs"] = round(med("pairs") / med("solve_nrhs"), 4)
res["backward_over_solve_nrhs"] = round(med("backward") / med("solve_nrhs"), 3)
res["torch_index_over_pairs"] = round(med("torch_index") / med("pairs"), 2)
res["torch_index_add_over_pairs"] = round(med("torch_index_add") / med("pairs"), 2)
pair_bytes = nzv * (4 * 8 * nrhs + 4 + 4 + 1 + 8)
res["pairs_gather_bytes"] = pair_bytes
res["pairs_gather_GBps"] = round(pair_bytes / (med("pairs") * 1e-3) / 1e9, 1)
dev.values_grad_pairs(Lam, X, alpha=-1.0, out=g)
ref = torch_index()
res["pairs_vs_torch_index_rel"] = float((g - ref).abs().max() / ref.abs().max())
print(json.dumps(res))
