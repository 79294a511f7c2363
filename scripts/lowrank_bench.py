"""Low-rank corrections on a factored A: cholamd_lowrank_set, the corrected solves against the plain ones, and what a user had before (development aid;
bench.py is the contract).

python scripts/lowrank_bench.py CASE K NRHS [reps]
  CASE = a fixture under tests/golden, gen:NXxNYxNZ:levels:tile or gen:N:levels (an N^3 grid, tile 64); K = columns of U; NRHS = right-hand sides of the
  block solves.  fp64 factor, update mode (C = I + U^T A^-1 U is positive definite for any U).  Everything is timed with HIP events on one stream: one
  warm-up round, then `reps` rounds in which every variant runs ONCE, in turn (interleaved repetitions), each between its own pair of events; reported as
  median [min, max] in ms, beside the mean time of an empty event pair (cholamd_device_event_overhead).  Variants:
    set              cholamd_lowrank_set (synchronises inside)
    solve_plain      cholamd_solve                      solve_lowrank       cholamd_lowrank_solve
    solve_nrhs_plain cholamd_solve_nrhs, NRHS columns   solve_nrhs_lowrank  cholamd_lowrank_solve_nrhs
    diag             cholamd_lowrank_diag (one pass over W)
    k_solves         what a user had before: K cholamd_solve calls on the columns of U and the download of the n x K result
  Derived: the correction's time (corrected - plain, medians) and the bytes of W it moves (2 n K doubles per chunk of 32 columns) over that time as a share
  of the HBM rate a copy kernel reaches on this chip (6.29e12 B/s); the same for diag (n K doubles).  Prints one JSON line."""
import json
import os
import statistics
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import torch  # noqa: E402

import cholesky_amd as ca  # noqa: E402

HBM_COPY_RATE = 6.29e12
case = sys.argv[1] if len(sys.argv) > 1 else "lapl_3375x3375"
k = int(sys.argv[2]) if len(sys.argv) > 2 else 64
nrhs = int(sys.argv[3]) if len(sys.argv) > 3 else 32
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 10
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
n = plan.n
arena = dev.new_arena()
dev.fill(arena)
dev.factor(arena)
dev.sync()
assert dev.info() == (0, 0), dev.info()
stream = torch.cuda.current_stream()


def cm(rows, cols):
    t = torch.empty((cols, rows), dtype=torch.float64, device="cuda").T
    t.copy_(torch.rand((rows, cols), dtype=torch.float64, device="cuda") - 0.5)
    return t


U, V, B, X = cm(n, k), cm(n, k), cm(n, nrhs), cm(n, nrhs)
b, x = B[:, 0].contiguous(), torch.empty(n, dtype=torch.float64, device="cuda")
w = torch.empty(n, dtype=torch.float64, device="cuda")
low = ca.LowRank(dev, k)
low.set(arena, U, "update")


def k_solves():
    for j in range(k):
        dev.solve(arena, U[:, j], V[:, j])
    return V.T.cpu()                                   # the download of n x K (the columns are contiguous)


variants = {
    "set": lambda: low.set(arena, U, "update"),
    "solve_plain": lambda: dev.solve(arena, b, x),
    "solve_lowrank": lambda: low.solve(arena, b, x),
    "solve_nrhs_plain": lambda: dev.solve_nrhs(arena, B, X),
    "solve_nrhs_lowrank": lambda: low.solve_nrhs(arena, B, X),
    "diag": lambda: low.diag(out=w),
    "k_solves": k_solves,
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


res = dict(case=case, n=n, k=k, nrhs=nrhs, reps=reps, device=torch.cuda.get_device_name(0), event_pair_ms=round(dev.event_overhead_ms(), 4))
for name, v in times.items():
    res[name + "_ms"] = stats(v)
med = lambda key: res[key + "_ms"]["median"]  # noqa: E731
chunks = (nrhs + 31) // 32
corr1, corrn = med("solve_lowrank") - med("solve_plain"), med("solve_nrhs_lowrank") - med("solve_nrhs_plain")
res["correction_ms"] = round(corr1, 4)
res["correction_nrhs_ms"] = round(corrn, 4)
res["w_bytes_per_pass"] = 8 * n * k
if corr1 > 0:
    res["correction_share_of_hbm"] = round(2 * 8 * n * k / (corr1 * 1e-3) / HBM_COPY_RATE, 4)
if corrn > 0:
    res["correction_nrhs_share_of_hbm"] = round(2 * chunks * 8 * n * k / (corrn * 1e-3) / HBM_COPY_RATE, 4)
res["diag_share_of_hbm"] = round(8 * n * k / (med("diag") * 1e-3) / HBM_COPY_RATE, 4)
res["solve_lowrank_over_plain"] = round(med("solve_lowrank") / med("solve_plain"), 3)
res["solve_nrhs_lowrank_over_plain"] = round(med("solve_nrhs_lowrank") / med("solve_nrhs_plain"), 3)
res["k_solves_over_set"] = round(med("k_solves") / med("set"), 2)
print(json.dumps(res))
low.close()
