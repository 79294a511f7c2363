"""The Schur complement path against the complete factorisation and the plain solve (development aid; bench.py is the contract).

python scripts/schur_bench.py CASE K [reps]
  CASE = a fixture under tests/golden, gen:NXxNYxNZ:levels:tile or gen:N:levels (an N^3 grid, tile 64); K = kept tree levels.  Everything is timed
  with HIP events on one stream: a warm-up call, then `reps` repeats, each between its own pair of events; reported as median [min, max] in ms.
  Measured: cholamd_device_fill + cholamd_factor (the parent's path), fill + cholamd_schur_factor, cholamd_schur alone (with the bytes it moves: the
  stored pieces read once, S written once), cholamd_solve on the complete factor, cholamd_schur_condense and cholamd_schur_expand (x_T from the
  complete solve, so that the numbers are those of a real right-hand side).  Prints one JSON line."""
import json
import os
import statistics
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import torch  # noqa: E402

import cholesky_amd as ca  # noqa: E402

case = sys.argv[1] if len(sys.argv) > 1 else "lapl_3375x3375"
k = int(sys.argv[2]) if len(sys.argv) > 2 else 1
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
n, m = plan.n, plan.schur_size(k)
full, part = dev.new_arena(), dev.new_arena()
S = torch.empty(m, m, dtype=torch.float64, device="cuda").T
stream = torch.cuda.current_stream()


def stats(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def timed(fn, reps=reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b))
    return stats(out)


def factor():
    dev.fill(full)
    dev.factor(full)


def schur_factor():
    dev.fill(part)
    dev.schur_factor(part, k)


res = dict(case=case, n=n, k=k, m=m, reps=reps, device=torch.cuda.get_device_name(0), fill_factor_ms=timed(factor))
dev.sync()
assert dev.info() == (0, 0), dev.info()
res["fill_schur_factor_ms"] = timed(schur_factor)
dev.sync()
assert dev.info() == (0, 0), dev.info()
res["schur_ms"] = timed(lambda: dev.schur(part, k, out=S))
rec = plan.schur_list(k)
moved = 8 * (int((rec[:, 2] * rec[:, 3]).sum()) + m * m)
res["schur_mbytes"] = round(moved * 1e-6, 3)
res["schur_gbytes_per_s"] = round(moved * 1e-6 / res["schur_ms"]["median"], 1)
res["schur_path_over_factor"] = round((res["fill_schur_factor_ms"]["median"] + res["schur_ms"]["median"]) / res["fill_factor_ms"]["median"], 3)
b = torch.rand(n, dtype=torch.float64, device="cuda") + 1.0
x, w, g, x2 = (torch.empty(c, dtype=torch.float64, device="cuda") for c in (n, n, m, n))
res["solve_ms"] = timed(lambda: dev.solve(full, b, x))
xt = x[torch.from_numpy(plan.schur_dofs(k).astype("int64")).cuda()].contiguous()
res["condense_ms"] = timed(lambda: dev.schur_condense(part, k, b, w=w, g=g))
res["expand_ms"] = timed(lambda: dev.schur_expand(part, k, w, xt, x=x2))
dev.sync()
res["condense_expand_over_solve"] = round((res["condense_ms"]["median"] + res["expand_ms"]["median"]) / res["solve_ms"]["median"], 3)
res["expand_vs_solve_rel"] = float((x2 - x).abs().max() / x.abs().max())
print(json.dumps(res))
