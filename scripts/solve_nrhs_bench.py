"""Block solve against single solves (development aid; bench.py is the contract).

python scripts/solve_nrhs_bench.py CASE [fp64|mixed] [reps]
  CASE = a fixture under tests/golden or gen:NXxNYxNZ:levels:tile.  For k in {1, 4, 16, 32, 64}, warmed up and timed with a device synchronise:
  one cholamd_solve (_f32 for mixed), k of them back to back, one cholamd_solve_nrhs (_f32) with k columns.  Prints one JSON line: ms, ms per
  right-hand side, and the bytes of the stored tiles of L per sweep over the time of each."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import cholesky_amd as ca

case = sys.argv[1] if len(sys.argv) > 1 else "lapl_3375x3375"
prec = sys.argv[2] if len(sys.argv) > 2 else "fp64"
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
assert prec in ("fp64", "mixed"), prec
if case.startswith("gen:"):
    _, dims, lv, tile = case.split(":")
    nx, ny, nz = (int(v) for v in dims.split("x"))
    plan = ca.Problem(nx, ny, nz, int(lv), int(tile)).plan()
else:
    G = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", case)
    files = sorted(os.listdir(G))
    mtx = [f for f in files if f.startswith("lapl") and f.endswith(".mtx")][0]
    plan = ca.Plan(os.path.join(G, mtx), os.path.join(G, [f for f in files if "_ord_" in f][0]), os.path.join(G, [f for f in files if "_clust_" in f][0]))
dev = ca.Device(plan, 0)
f32 = prec == "mixed"
if f32:
    arena = dev.new_arena_f32()
    dev.fill_f32(arena)
    dev.factor_f32(arena)
else:
    arena = dev.new_arena()
    dev.fill(arena)
    dev.factor(arena)
dev.sync()
assert dev.info() == (0, 0), dev.info()
n, KS = plan.n, (1, 4, 16, 32, 64)
bytes_sweep = plan.nnz_tiles * (4 if f32 else 8)  # the stored tiles of L, read once per sweep
g = torch.Generator(device="cuda").manual_seed(1)
B = torch.randn(max(KS), n, dtype=torch.float64, device="cuda", generator=g).T
X = torch.empty(max(KS), n, dtype=torch.float64, device="cuda").T
single = dev.solve_f32 if f32 else dev.solve


def timed(fn):
    fn()
    dev.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    dev.sync()
    return (time.perf_counter() - t0) * 1e3 / reps


def singles(k):
    for j in range(k):
        single(arena, B[:, j], X[:, j])


one = timed(lambda: single(arena, B[:, 0], X[:, 0]))
rows = []
for k in KS:
    t_single = timed(lambda: singles(k))
    t_block = timed(lambda: dev.solve_nrhs(arena, B[:, :k], X[:, :k]))
    sweeps = 2 * ((k + 31) // 32)  # forward + backward per 32-column chunk
    rows.append(dict(k=k, singles_ms=round(t_single, 3), nrhs_ms=round(t_block, 3), nrhs_ms_per_rhs=round(t_block / k, 4),
                     nrhs_over_one_solve=round(t_block / one, 2), speedup_vs_singles=round(t_single / t_block, 2),
                     nrhs_factor_TBps=round(bytes_sweep * sweeps / (t_block * 1e-3) / 1e12, 3)))
print(json.dumps(dict(case=case, precision=prec, n=n, factor_bytes_per_sweep=int(bytes_sweep), one_solve_ms=round(one, 3),
                      one_solve_factor_TBps=round(2 * bytes_sweep / (one * 1e-3) / 1e12, 3), rows=rows)))
