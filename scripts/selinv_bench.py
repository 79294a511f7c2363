"""Selected inversion against the factorisation and against probing with unit vectors (development aid; bench.py is the contract).

python scripts/selinv_bench.py CASE [reps] [--full-probe]
  CASE = a fixture under tests/golden, gen:NXxNYxNZ:levels:tile or gen:N:levels (an N^3 grid, tile 64).  Everything is timed with HIP events on one
  stream: a warm-up call, then `reps` repeats, each between its own pair of events; reported as median [min, max] in ms.  Measured: cholamd_device_fill
  + cholamd_factor, cholamd_selinv, cholamd_selinv_diag beside cholamd_factor_diag, cholamd_selinv_entries beside cholamd_device_set_values (no check),
  one 32-column chunk of cholamd_solve_nrhs on unit vectors and the diagonal by probing as chunk time x ceil(n / 32) -- or timed in full with
  --full-probe.  Prints one JSON line."""
import json
import os
import statistics
import sys

args = [a for a in sys.argv[1:]]
full_probe = "--full-probe" in args
args = [a for a in args if a != "--full-probe"]
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import torch  # noqa: E402

import cholesky_amd as ca  # noqa: E402

case = args[0] if len(args) > 0 else "lapl_3375x3375"
reps = int(args[1]) if len(args) > 1 else 10
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
arena, z = dev.new_arena(), dev.new_arena()
n = plan.n
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
    dev.fill(arena)
    dev.factor(arena)


res = dict(case=case, n=n, reps=reps, arena_doubles=plan.arena_doubles, fill_factor_ms=timed(factor))
dev.sync()
assert dev.info() == (0, 0), dev.info()
res["selinv_ms"] = timed(lambda: dev.selinv(arena, z))
# useful flops of the gather-product Z[below, J] = -Z[below, below] Y: 2 m^2 nb per column block with m rows below it (host view, counts only)
gflop = 0.0
for sep in range(1, plan.nsep + 1):
    w = int(plan.sep_sizes[sep - 1])
    for blk in range(plan.selinv_blocks(sep)):
        m = plan.L.cholamd_plan_selinv_front(plan.h, sep, blk, 0, None, None, None)
        gflop += 2.0 * m * m * min(64, w - 64 * blk) * 1e-9
res["gather_gflop"] = round(gflop, 3)
res["selinv_over_factor"] = round(res["selinv_ms"]["median"] / res["fill_factor_ms"]["median"], 2)
diag = torch.empty(n, dtype=torch.float64, device="cuda")
vals = torch.empty(plan.nz, dtype=torch.float64, device="cuda")
res["selinv_diag_ms"] = timed(lambda: dev.selinv_diag(z, out=diag))
res["factor_diag_ms"] = timed(lambda: dev.factor_diag(arena, out=diag))
res["selinv_entries_ms"] = timed(lambda: dev.selinv_entries(z, out=vals))
res["set_values_nocheck_ms"] = timed(lambda: dev.set_values(vals.nan_to_num(1.0), check=False))
# the route without selected inversion: unit vectors through the block solve, 32 at a time
E = torch.zeros(32, n, dtype=torch.float64, device="cuda").T
E[torch.arange(32), torch.arange(32)] = 1.0
X = torch.empty(32, n, dtype=torch.float64, device="cuda").T
res["probe_chunk_ms"] = timed(lambda: dev.solve_nrhs(arena, E, X))
chunks = (n + 31) // 32
res["probe_diag_estimate_ms"] = round(res["probe_chunk_ms"]["median"] * chunks, 1)
if full_probe:
    def probe():
        for c in range(chunks):
            dev.solve_nrhs(arena, E, X)
    res["probe_diag_full_ms"] = timed(probe, reps=max(1, reps // 5))
print(json.dumps(res))
