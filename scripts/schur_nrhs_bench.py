"""Schur condense + expand for many right-hand sides: the block calls and the option schur_deterministic against the single-vector calls (development
aid; bench.py is the contract).

python scripts/schur_nrhs_bench.py CASE PRECISION K NRHS [reps]
  CASE = a fixture under tests/golden, gen:NXxNYxNZ:levels:tile or gen:N:levels (an N^3 grid, tile 64); PRECISION = fp64 | fp32 (the arena's element
  type); K = kept tree levels; NRHS = columns.  Everything is timed with HIP events on one stream: a warm-up call, then `reps` repeats, each between its
  own pair of events; reported as median [min, max] in ms.  Measured, each as condense + expand of all NRHS columns:
    single_atomic   NRHS calls of cholamd_schur_condense and of cholamd_schur_expand, option off (the path before the block calls existed)
    block_atomic    one cholamd_schur_condense_nrhs and one cholamd_schur_expand_nrhs, option off
    block_det       the same with schur_deterministic on
  and for one column: single1_atomic, single1_det (cholamd_schur_condense + cholamd_schur_expand, option off / on).  XT is G itself: the time of a sweep
  does not depend on the values.  Prints one JSON line with the ratios."""
import json
import os
import statistics
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import torch  # noqa: E402

import cholesky_amd as ca  # noqa: E402

case = sys.argv[1] if len(sys.argv) > 1 else "lapl_3375x3375"
f32 = (sys.argv[2] if len(sys.argv) > 2 else "fp64") == "fp32"
k = int(sys.argv[3]) if len(sys.argv) > 3 else 1
nrhs = int(sys.argv[4]) if len(sys.argv) > 4 else 32
reps = int(sys.argv[5]) if len(sys.argv) > 5 else 10
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
if f32:
    arena = dev.new_arena_f32()
    dev.fill_f32(arena)
    dev.factor_levels_f32(arena, plan.levels - 1, k)
else:
    arena = dev.new_arena()
    dev.fill(arena)
    dev.schur_factor(arena, k)
dev.sync()
assert dev.info() == (0, 0), dev.info()
stream = torch.cuda.current_stream()


def stats(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def timed(fn):
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


def cm(rows):
    return torch.empty((nrhs, rows), dtype=torch.float64, device="cuda").T


B = cm(n)
B.copy_(torch.rand((n, nrhs), dtype=torch.float64, device="cuda") + 1.0)
W, Gm, X = cm(n), cm(m), cm(n)
cols = [tuple(t[:, j] for t in (B, W, Gm, X)) for j in range(nrhs)]      # column views: contiguous vectors


def single(count):
    for b, w, g, x in cols[:count]:
        dev.schur_condense(arena, k, b, w=w, g=g)
    for b, w, g, x in cols[:count]:
        dev.schur_expand(arena, k, w, g, x=x)


def block():
    dev.schur_condense_nrhs(arena, k, B, W=W, G=Gm)
    dev.schur_expand_nrhs(arena, k, W, Gm, X=X)


res = dict(case=case, precision="fp32" if f32 else "fp64", n=n, k=k, m=m, nrhs=nrhs, reps=reps, device=torch.cuda.get_device_name(0))
dev.set_option("schur_deterministic", 0)
res["single_atomic_ms"] = timed(lambda: single(nrhs))
res["single1_atomic_ms"] = timed(lambda: single(1))
res["block_atomic_ms"] = timed(block)
x_atomic = X.clone()
dev.set_option("schur_deterministic", 1)
res["block_det_ms"] = timed(block)
res["single1_det_ms"] = timed(lambda: single(1))
dev.sync()
res["block_det_vs_atomic_rel"] = float((X - x_atomic).abs().max() / x_atomic.abs().max())
med = lambda key: res[key]["median"]  # noqa: E731
res["single_over_block_atomic"] = round(med("single_atomic_ms") / med("block_atomic_ms"), 2)
res["single_over_block_det"] = round(med("single_atomic_ms") / med("block_det_ms"), 2)
res["block_det_over_block_atomic"] = round(med("block_det_ms") / med("block_atomic_ms"), 2)
res["single1_det_over_atomic"] = round(med("single1_det_ms") / med("single1_atomic_ms"), 2)
res["launches"] = dev.schur_launches()
res["copy_mbytes_per_chunk"] = round(8 * 32 * (2 * n + m) * 1e-6, 3)      # unpack: the block read, W and G written; pack moves the same
print(json.dumps(res))
