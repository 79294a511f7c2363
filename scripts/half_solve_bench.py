"""Half solves, logdet and factor_diag against the full solve (development aid; bench.py is the contract).

python scripts/half_solve_bench.py CASE [fp64|mixed] [reps] [--root TREE]
  CASE = a fixture under tests/golden, gen:NXxNYxNZ:levels:tile or gen:N:levels (an N^3 grid, tile 64).  Everything is timed with HIP events on one stream: a warm-up call, then `reps`
  repeats, each between its own pair of events; reported as median [min, max] in ms.  Measured: one cholamd_solve (_f32 for mixed), FORWARD, BACKWARD,
  FORWARD then BACKWARD; block halves at k = 4, 16, 32, 64 against k single halves; cholamd_factor_diag (events) and cholamd_factor_logdet (host wall
  clock: the call synchronises).  --root TREE imports cholesky_amd from another built tree (a parent commit's build, for its cholamd_solve in the same
  session); a library without the half solves reports the solve alone.  Prints one JSON line."""
import json
import os
import statistics
import sys
import time

args = [a for a in sys.argv[1:]]
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in args:
    i = args.index("--root")
    root = os.path.abspath(args[i + 1])
    del args[i:i + 2]
sys.path.insert(0, root)
import torch  # noqa: E402

import cholesky_amd as ca  # noqa: E402

case = args[0] if len(args) > 0 else "lapl_3375x3375"
prec = args[1] if len(args) > 1 else "fp64"
reps = int(args[2]) if len(args) > 2 else 20
assert prec in ("fp64", "mixed"), prec
if case.startswith("gen:"):
    parts = case.split(":")
    dims, lv, tile = parts[1], parts[2], parts[3] if len(parts) > 3 else 64      # gen:N:levels = an N^3 grid, tile 64
    nx, ny, nz = (int(v) for v in dims.split("x")) if "x" in dims else (int(dims),) * 3
    plan = ca.Problem(nx, ny, nz, int(lv), int(tile)).plan()
else:
    G = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", case)
    files = sorted(os.listdir(G))
    mtx = [f for f in files if f.startswith("lapl") and f.endswith(".mtx")][0]
    plan = ca.Plan(os.path.join(G, mtx), os.path.join(G, [f for f in files if "_ord_" in f][0]), os.path.join(G, [f for f in files if "_clust_" in f][0]))
dev = ca.Device(plan, 0)
f32 = prec == "mixed"
arena = dev.new_arena_f32() if f32 else dev.new_arena()
(dev.fill_f32 if f32 else dev.fill)(arena)
(dev.factor_f32 if f32 else dev.factor)(arena)
dev.sync()
assert dev.info() == (0, 0), dev.info()
n, KS = plan.n, (4, 16, 32, 64)
g = torch.Generator(device="cuda").manual_seed(1)
B = torch.randn(max(KS), n, dtype=torch.float64, device="cuda", generator=g).T
X = torch.empty(max(KS), n, dtype=torch.float64, device="cuda").T
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


def wall(fn):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return stats(out)


single = dev.solve_f32 if f32 else dev.solve
res = dict(case=case, precision=prec, n=n, reps=reps, root=root, solve_ms=timed(lambda: single(arena, B[:, 0], X[:, 0])))
if hasattr(dev, "solve_half"):
    FWD, BWD = ca.HALF_FORWARD, ca.HALF_BACKWARD
    res["forward_ms"] = timed(lambda: dev.solve_half(arena, B[:, 0], X[:, 0], FWD))
    res["backward_ms"] = timed(lambda: dev.solve_half(arena, B[:, 0], X[:, 0], BWD))

    def both():
        dev.solve_half(arena, B[:, 0], X[:, 0], FWD)
        dev.solve_half(arena, X[:, 0], X[:, 0], BWD)

    res["forward_then_backward_ms"] = timed(both)
    rows = []
    for k in KS:
        row = dict(k=k)
        for name, which in (("forward", FWD), ("backward", BWD)):
            def singles():
                for j in range(k):
                    dev.solve_half(arena, B[:, j], X[:, j], which)
            ts, tb = timed(singles), timed(lambda: dev.solve_half_nrhs(arena, B[:, :k], X[:, :k], which))
            row[name] = dict(singles_ms=ts, block_ms=tb, block_over_one_half=round(tb["median"] / res[name + "_ms"]["median"], 2),
                             speedup_vs_singles=round(ts["median"] / tb["median"], 2))
        rows.append(row)
    res["rows"] = rows
    diag = torch.empty(n, dtype=torch.float64, device="cuda")
    res["factor_diag_ms"] = timed(lambda: dev.factor_diag(arena, out=diag))
    res["logdet_wall_ms"] = wall(lambda: dev.logdet(arena))
    res["solve_wall_ms"] = wall(lambda: (single(arena, B[:, 0], X[:, 0]), dev.sync()))
    res["diag_estimate_ms"] = round(n * 64 / 6.3e12 * 1e3, 5)     # n sectors of 64 B at 6.3 TB/s
print(json.dumps(res))
