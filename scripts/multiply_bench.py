#!/usr/bin/env python3
"""Times of the factor applied forwards against the solves that read the same bytes.

  python scripts/multiply_bench.py CASE PRECISION [NRHS]   CASE: lapl_3375 | gen:NX:LEVELS (an NX^3 grid);  PRECISION: fp64 | fp32

HIP events on one stream around every call, a warm-up, then the median [min, max] over 30 repeats (lapl_3375) or 8 (generated grids).  Reported:
multiply_half both ways against cholamd_solve_half of the same `which` (timed in the same process), with the bytes of L the product reads divided by
the time as a fraction of the HBM peak (the bytes are counted from the product's own lists, Plan.multiply_counts: lower triangles only, the leaf skips
left out); multiply against solve; factor_residual against residual (both synchronise: host timer); the list sizes and the first call's time (list
build and upload).

With NRHS the block form is timed too (multiply_half_nrhs both ways, multiply_nrhs), all in the same process: the single product (the unchanged k_multiply),
NRHS single calls in a loop, the block call of NRHS columns on the default path, with every chunk forced onto the block kernel (option multiply_nrhs_min
= 1) and forced column by column (= 33), a forced block chunk of 32 columns and one of 1 column; bytes of L per time for the 32-column chunk (one pass), and
min = ceil(T_chunk(32 columns) / T_single), the threshold multiply_nrhs_min_block of chol_api_query.cpp takes at gen:60:8."""
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
    if len(sys.argv) > 3:
        block_form(dev, a, n, int(sys.argv[3]), timed, l_bytes)


def block_form(dev, a, n, nrhs, timed, l_bytes):
    import math
    import torch
    kmax = max(nrhs, 32)
    Z = torch.randn(kmax, n, dtype=torch.float64, device="cuda").T
    Y = torch.empty(kmax, n, dtype=torch.float64, device="cuda").T
    fmt = lambda t: f"{t[0]:9.3f} ms [{t[1]:.3f}, {t[2]:.3f}]"  # noqa: E731
    print(f"block form, nrhs = {nrhs}:")
    for tag, which in (("FORWARD", 0), ("BACKWARD", 1), ("full", None)):
        if which is None:
            one = lambda j: dev.multiply(a, Z[:, j], Y[:, j])  # noqa: E731
            blk = lambda k: dev.multiply_nrhs(a, Z[:, :k], Y[:, :k])  # noqa: E731
            nbytes = l_bytes[0] + l_bytes[1]
        else:
            one = lambda j, w=which: dev.multiply_half(a, Z[:, j], Y[:, j], w)  # noqa: E731
            blk = lambda k, w=which: dev.multiply_half_nrhs(a, Z[:, :k], Y[:, :k], w)  # noqa: E731
            nbytes = l_bytes[which]

        def loop(k):
            for j in range(k):
                one(j)

        t_single = timed(lambda: one(0))
        t_loop = timed(lambda: loop(nrhs))
        dev.set_option("multiply_nrhs_min", 0)
        t_default = timed(lambda: blk(nrhs))
        dev.set_option("multiply_nrhs_min", 33)
        t_cols = timed(lambda: blk(nrhs))
        dev.set_option("multiply_nrhs_min", 1)
        t_block = timed(lambda: blk(nrhs))
        t_32 = timed(lambda: blk(32))
        t_1 = timed(lambda: blk(1))
        dev.set_option("multiply_nrhs_min", 0)
        print(f"  {tag:9s} single product        {fmt(t_single)}")
        print(f"  {tag:9s} {nrhs:3d} single calls      {fmt(t_loop)}")
        print(f"  {tag:9s} block call, default   {fmt(t_default)}")
        print(f"  {tag:9s} block call, forced    {fmt(t_block)}")
        print(f"  {tag:9s} block call, columns   {fmt(t_cols)}")
        print(f"  {tag:9s} 32-column chunk       {fmt(t_32)}   {nbytes / (t_32[0] * 1e-3) / 1e12:.3f} TB/s = {nbytes / (t_32[0] * 1e-3) / HBM_PEAK:.1%} of peak")
        print(f"  {tag:9s} forced 1-column chunk {fmt(t_1)}")
        print(f"  {tag:9s} min = ceil(T_chunk(32) / T_single) = {math.ceil(t_32[0] / t_single[0])};  32 columns: block / single calls = {t_block[0] / t_loop[0]:.3f}" if nrhs == 32 else
              f"  {tag:9s} min = ceil(T_chunk(32) / T_single) = {math.ceil(t_32[0] / t_single[0])}")


if __name__ == "__main__":
    main()
