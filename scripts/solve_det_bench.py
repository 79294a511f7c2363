#!/usr/bin/env python3
"""Times of the deterministic streamed solve against the atomic streamed solve and solve_reference_shape.

  python scripts/solve_det_bench.py CASE PRECISION   CASE: lapl_3375 | gen:NX:LEVELS (an NX^3 grid);  PRECISION: fp64 | fp32

HIP events on one stream around every call, a warm-up of every path, then the median [min, max] over 30 repeats (lapl_3375) or 8 (generated grids).  The
paths run ALTERNATELY in one process on one device object and one arena -- repeat r times the deterministic solve (option solve_deterministic), then the
atomic one (both options off), then solve_reference_shape (fp64 factor only: the option does not apply to an fp32 factor) -- for the solve and for both
halves.  Reported besides: launches per sweep (one span launch per step that has a span plus one gather launch per step that has items; the permutes and the 16x16
inverses come on top for every path), the entries of L a sweep reads (Plan.solve_det_counts) and those bytes over the time as a fraction of the HBM peak.

THE CONDITION (fp64): the deterministic solve is faster than solve_reference_shape by more than the two spreads -- its slowest repeat below the other's
fastest.  The last line says whether it holds.

  python scripts/solve_det_bench.py CASE PRECISION NRHS   the BLOCK form on NRHS right-hand sides (DESIGN.md section 14 at "Block form")

With NRHS the call is solve_nrhs on an n x NRHS block and three paths alternate in the same way: the deterministic block solve (options solve_deterministic
and solve_deterministic_block), the deterministic column-wise solve (solve_deterministic alone: one single-vector solve per column) and the atomic block
solve (both off).  Bytes: the entries of L once per chunk of 32 columns.  ITS CONDITION: the block solve's slowest repeat below the column-wise solve's
fastest."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12   # bytes / s, MI355X


def main():
    import torch
    import cholesky_amd as ca
    case, prec = sys.argv[1], sys.argv[2]
    f32 = prec == "fp32"
    if case == "lapl_3375":
        d = os.path.join(ROOT, "tests", "golden", "lapl_3375x3375")
        plan = ca.Plan(os.path.join(d, "lapl_15_3.mtx"), os.path.join(d, "lapl_15_3_ord_5.txt"), os.path.join(d, "lapl_15_3_clust_5.txt"))
        reps = 30
    else:
        _, nx, levels = case.split(":")
        plan = ca.Problem(int(nx), int(nx), int(nx), levels=int(levels), tile=64).plan()
        reps = 8
    dev = ca.Device(plan, 0)
    a = dev.new_arena_f32() if f32 else dev.new_arena()
    (dev.fill_f32 if f32 else dev.fill)(a)
    (dev.factor_f32 if f32 else dev.factor)(a)
    dev.sync()
    assert dev.info() == (0, 0)
    n = plan.n
    nrhs = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    b = torch.randn(n, dtype=torch.float64, device="cuda")
    x = torch.empty_like(b)
    t0 = time.perf_counter()
    cnt = plan.solve_det_counts()
    t_lists = 1e3 * (time.perf_counter() - t0)
    esz = 4 if f32 else 8
    launches = {}
    for which, w in ((0, "forward"), (1, "backward")):
        steps, _, _ = plan.solve_det_lists(which)
        launches[w] = int((steps[:, 1] >= 0).sum()) + int((steps[:, 3] > steps[:, 2]).sum())
    paths = [("deterministic", {"solve_deterministic": 1, "solve_reference_shape": 0}), ("atomic", {"solve_deterministic": 0, "solve_reference_shape": 0})]
    if not f32:
        paths.append(("reference_shape", {"solve_deterministic": 0, "solve_reference_shape": 1}))
    solve = dev.solve_f32 if f32 else dev.solve
    if nrhs > 0:
        block_bench(dev, a, plan, cnt, case, prec, nrhs, reps)
        return
    calls = [("solve", lambda: solve(a, b, x)), ("half FORWARD", lambda: dev.solve_half(a, b, x, 0)), ("half BACKWARD", lambda: dev.solve_half(a, b, x, 1))]

    def use(opts):
        for k, v in opts.items():
            dev.set_option(k, v)

    print(f"{case} {prec}: n = {n}, {reps} repeats; the lists on the host take {t_lists:.1f} ms to build")
    for w in ("forward", "backward"):
        c = cnt[w]
        print(f"  {w}: {c['steps']} steps, {launches[w]} launches per sweep, {c['items']} items, {c['sources']} sources ({24 * c['sources'] / 1e6:.2f} MB of list), "
              f"{c['entries']} entries = {c['entries'] * esz / 1e6:.1f} MB of L read")
    results = {}
    for tag, fn in calls:
        ts = {p: [] for p, _ in paths}
        for p, opts in paths:                       # warm-up: lists built and uploaded, kernels loaded
            use(opts)
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        for _ in range(reps):
            for p, opts in paths:
                use(opts)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts[p].append(e0.elapsed_time(e1))
        nbytes = esz * {"solve": cnt["forward"]["entries"] + cnt["backward"]["entries"], "half FORWARD": cnt["forward"]["entries"],
                        "half BACKWARD": cnt["backward"]["entries"]}[tag]
        for p, _ in paths:
            t = (statistics.median(ts[p]), min(ts[p]), max(ts[p]))
            results[tag, p] = t
            print(f"{tag:14s} {p:16s} {t[0]:10.3f} ms [{t[1]:.3f}, {t[2]:.3f}]   {nbytes / (t[0] * 1e-3) / 1e12:.3f} TB/s = {nbytes / (t[0] * 1e-3) / HBM_PEAK:.1%} of peak")
        d, at = results[tag, "deterministic"], results[tag, "atomic"]
        print(f"{tag:14s} deterministic / atomic = {d[0] / at[0]:.2f}")
    use(paths[1][1])
    if not f32:
        d, r = results["solve", "deterministic"], results["solve", "reference_shape"]
        ok = d[2] < r[1]
        print(f"condition (the deterministic solve's slowest repeat {d[2]:.3f} ms below solve_reference_shape's fastest {r[1]:.3f} ms): {'HOLDS' if ok else 'FAILS'}")


def block_bench(dev, a, plan, cnt, case, prec, nrhs, reps):
    import torch
    n, esz = plan.n, 4 if prec == "fp32" else 8
    B = torch.randn(nrhs, n, dtype=torch.float64, device="cuda").T      # column-major n x nrhs
    X = torch.empty(nrhs, n, dtype=torch.float64, device="cuda").T
    paths = [("det block", {"solve_deterministic": 1, "solve_deterministic_block": 1}), ("det column-wise", {"solve_deterministic": 1, "solve_deterministic_block": 0}),
             ("atomic block", {"solve_deterministic": 0, "solve_deterministic_block": 0})]
    dev.set_option("solve_reference_shape", 0)
    chunks = (nrhs + 31) // 32
    nbytes = esz * chunks * (cnt["forward"]["entries"] + cnt["backward"]["entries"])
    print(f"{case} {prec}: n = {n}, solve_nrhs of {nrhs} columns ({chunks} chunks of 32), {reps} repeats")
    ts = {p: [] for p, _ in paths}
    for p, opts in paths:                           # warm-up: lists built and uploaded, kernels loaded
        for k, v in opts.items():
            dev.set_option(k, v)
        for _ in range(2):
            dev.solve_nrhs(a, B, X)
    torch.cuda.synchronize()
    for _ in range(reps):
        for p, opts in paths:
            for k, v in opts.items():
                dev.set_option(k, v)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dev.solve_nrhs(a, B, X)
            e1.record()
            e1.synchronize()
            ts[p].append(e0.elapsed_time(e1))
    res = {}
    for p, _ in paths:
        t = res[p] = (statistics.median(ts[p]), min(ts[p]), max(ts[p]))
        print(f"solve_nrhs({nrhs:3d}) {p:16s} {t[0]:10.3f} ms [{t[1]:.3f}, {t[2]:.3f}]   {t[0] / nrhs:8.4f} ms per column   "
              f"{nbytes / (t[0] * 1e-3) / 1e12:.3f} TB/s = {nbytes / (t[0] * 1e-3) / HBM_PEAK:.1%} of peak (the bytes of L per chunk)")
    for k in ("solve_deterministic", "solve_deterministic_block"):
        dev.set_option(k, 0)
    d, c, at = res["det block"], res["det column-wise"], res["atomic block"]
    print(f"det block / atomic block = {d[0] / at[0]:.2f}, det column-wise / det block = {c[0] / d[0]:.2f}")
    print(f"condition (the block solve's slowest repeat {d[2]:.3f} ms below the column-wise solve's fastest {c[1]:.3f} ms): {'HOLDS' if d[2] < c[1] else 'FAILS'}")


if __name__ == "__main__":
    main()
