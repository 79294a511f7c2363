#!/usr/bin/env python3
"""Times of the factor applied forwards against the solves that read the same bytes.

  python scripts/multiply_bench.py CASE PRECISION        CASE: lapl_3375 | gen:NX:LEVELS (an NX^3 grid);  PRECISION: fp64 | fp32

HIP events on one stream around every call, a warm-up, then the median [min, max] over 30 repeats (lapl_3375) or 8 (generated grids).  Reported:
multiply_half both ways against cholamd_solve_half of the same `which` (timed in the same process), with the bytes of L the product reads divided by
the time as a fraction of the HBM peak (the bytes are counted from the product's own lists, Plan.multiply_counts: lower triangles only, the leaf skips
left out); multiply against solve; factor_residual against residual (both synchronise: host timer); the list sizes and the first call's time (list
build and upload)."""
import os
import statistics
import sys
import time

import numpy as np

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
    z = torch.randn(n, dtype=torch.float64, device="cuda")
    y = torch.empty_like(z)
    cnt = plan.multiply_counts()
    esz = 4 if f32 else 8
    l_bytes = {0: cnt["forward"]["entries"] * esz, 1: cnt["backward"]["entries"] * esz}   # what one product reads of L
    t0 = time.perf_counter()
    dev.multiply_half(a, z, y, 0)
    dev.sync()
    first = 1e3 * (time.perf_counter() - t0)

    def timed(fn, host=False):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            if host:
                t0 = time.perf_counter()
                fn()
                ts.append(1e3 * (time.perf_counter() - t0))
            else:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
        return statistics.median(ts), min(ts), max(ts)

    def row(tag, new, old, bytes_read=None):
        extra = f"  {bytes_read / (new[0] * 1e-3) / 1e12:.3f} TB/s = {bytes_read / (new[0] * 1e-3) / HBM_PEAK:.1%} of peak" if bytes_read else ""
        print(f"{tag:34s} {new[0]:9.3f} ms [{new[1]:.3f}, {new[2]:.3f}]   against {old[0]:9.3f} ms [{old[1]:.3f}, {old[2]:.3f}]{extra}")

    print(f"{case} {prec}: n = {n}, {reps} repeats; first call (lists built and uploaded) {first:.1f} ms")
    for w in ("forward", "backward"):
        c = cnt[w]
        print(f"  {w}: {c['items']} items, {c['sources']} sources ({24 * c['sources'] / 1e6:.2f} MB of list), {c['entries'] * esz / 1e6:.1f} MB of L read")
    for which, nm in ((0, "FORWARD"), (1, "BACKWARD")):
        row(f"multiply_half {nm} / solve_half", timed(lambda: dev.multiply_half(a, z, y, which)), timed(lambda: dev.solve_half(a, z, y, which)), l_bytes[which])
    solve = dev.solve_f32 if f32 else dev.solve
    row("multiply / solve", timed(lambda: dev.multiply(a, z, y)), timed(lambda: solve(a, z, y)), l_bytes[0] + l_bytes[1])
    row("factor_residual / residual", timed(lambda: dev.factor_residual(a, z), host=True), timed(lambda: dev.residual(z, y), host=True))


if __name__ == "__main__":
    main()
