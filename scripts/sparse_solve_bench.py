#!/usr/bin/env python3
"""Times of the sparse solve (cholesky_amd.SparseSolve) against the whole-tree block solve.

  python scripts/sparse_solve_bench.py CASE PRECISION NIN NOUT NRHS [NIN NOUT NRHS ...]   (further triples: on the same plan, device object and factor)
    CASE: lapl_3375 | gen:NX:LEVELS (an NX^3 grid);  PRECISION: fp64 | fp32
    NIN, NOUT: K (the first K dofs of the first leaf), rK (K dofs drawn over the whole grid, seeded) or all;  NRHS: columns of the call

HIP events on one stream around every call, a warm-up of every path, then the median [min, max] over 30 repeats (lapl_3375) or 8 (generated grids).  Three
paths alternate in one process on one device object and one arena: the sparse solve, Device.solve_nrhs of the scattered n x NRHS block with the atomic
kernels, and the same with both deterministic options.  Reported besides: the time of SparseSolve's creation (the pruned lists built on the host and
uploaded), the launches a call makes, and next to every time ratio the ratio of the entries of L read (SparseSolve.counts against Plan.solve_det_counts):
where the two diverge, the launch chain of the top separators' spans is what is left.  With NIN == NOUT of at most 32 dofs, inverse_block against that
many columns of the full block solve."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dofs_of(plan, spec, seed):
    if spec == "all":
        return np.arange(plan.n, dtype=np.int32)
    if spec.startswith("r"):
        return np.sort(np.random.default_rng(seed).choice(plan.n, size=int(spec[1:]), replace=False)).astype(np.int32)
    leaf = int(plan.tree[(1 << (plan.levels - 1)) - 1])
    o, m, k = int(plan.sep_offsets[leaf - 1]), int(plan.sep_sizes[leaf - 1]), int(spec)
    assert k <= m, f"the first leaf has {m} dofs"
    return np.asarray(plan.perm[o:o + k], dtype=np.int32)


def timed(fn, paths, reps):
    import torch
    ts = {p: [] for p, _ in paths}
    for p, pre in paths:                            # warm-up: lists built and uploaded, kernels loaded
        pre()
        for _ in range(2):
            fn[p]()
    torch.cuda.synchronize()
    for _ in range(reps):
        for p, pre in paths:
            pre()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn[p]()
            e1.record()
            e1.synchronize()
            ts[p].append(e0.elapsed_time(e1))
    return {p: (statistics.median(t), min(t), max(t)) for p, t in ts.items()}


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
    for k in range(3, len(sys.argv) - 2, 3):
        one(plan, dev, a, case, prec, reps, sys.argv[k], sys.argv[k + 1], int(sys.argv[k + 2]))


def one(plan, dev, a, case, prec, reps, s_in, s_out, nrhs):
    import torch
    import cholesky_amd as ca
    n = plan.n
    i, o = dofs_of(plan, s_in, 1), dofs_of(plan, s_out, 2 if s_out != s_in else 1)
    t0 = time.perf_counter()
    h = ca.SparseSolve(dev, i, o)
    t_create = 1e3 * (time.perf_counter() - t0)
    c, full = h.counts(), plan.solve_det_counts()
    launches = 2 * ((nrhs + 31) // 32)              # the load and the store of every chunk
    for q, w in ((0, "forward"), (1, "backward")):
        steps, _, _ = plan.sparse_lists(i, o, q)
        launches += ((nrhs + 31) // 32) * (int((steps[:, 1] >= 0).sum()) + int((steps[:, 3] > steps[:, 2]).sum()))
    print(f"{case} {prec}: n = {n}, {len(i)} in ({s_in}), {len(o)} out ({s_out}), {nrhs} columns, {reps} repeats; create {t_create:.1f} ms")
    for w in ("forward", "backward"):
        print(f"  {w}: {c[w]['separators']} of {plan.nsep} separators, {c[w]['steps']} of {full[w]['steps']} steps, {c[w]['items']} of {full[w]['items']} items, "
              f"{c[w]['entries']} of {full[w]['entries']} entries of L ({c[w]['entries'] / full[w]['entries']:.5f})")
    print(f"  {c['positions']} of {n} positions active in {c['ranges']} ranges; a call makes {launches} launches plus at most {plan.levels} for the 16x16 inverses")
    Bs = torch.randn(nrhs, len(i), dtype=torch.float64, device="cuda").T
    Xs = torch.empty(nrhs, len(o), dtype=torch.float64, device="cuda").T
    B = torch.zeros(nrhs, n, dtype=torch.float64, device="cuda").T
    B[torch.from_numpy(i.astype(np.int64)).cuda()] = Bs
    X = torch.empty(nrhs, n, dtype=torch.float64, device="cuda").T

    def options(det):
        def pre():
            dev.set_option("solve_reference_shape", 0)
            dev.set_option("solve_deterministic", det)
            dev.set_option("solve_deterministic_block", det)
        return pre
    paths = [("sparse", lambda: None), ("atomic block", options(0)), ("det block", options(1))]
    fn = {"sparse": lambda: h.solve_nrhs(a, Bs, Xs), "atomic block": lambda: dev.solve_nrhs(a, B, X), "det block": lambda: dev.solve_nrhs(a, B, X)}
    res = timed(fn, paths, reps)
    ratio_entries = (c["forward"]["entries"] + c["backward"]["entries"]) / (full["forward"]["entries"] + full["backward"]["entries"])
    for p, _ in paths:
        t = res[p]
        print(f"solve({nrhs:3d}) {p:14s} {t[0]:10.3f} ms [{t[1]:.3f}, {t[2]:.3f}]")
    s = res["sparse"][0]
    print(f"sparse / atomic block = {s / res['atomic block'][0]:.4f}, sparse / det block = {s / res['det block'][0]:.4f}; entries read: sparse / full = {ratio_entries:.5f}")
    err = float((Xs - X[torch.from_numpy(o.astype(np.int64)).cuda()]).abs().max() / X.abs().max())       # (X: the last det block solve)
    print(f"max |x_sparse - x_det block| / max |x| on the outputs = {err:.2e}")
    if np.array_equal(i, o) and len(i) <= 32:
        m = len(i)
        E = torch.zeros(m, n, dtype=torch.float64, device="cuda").T
        E[torch.from_numpy(i.astype(np.int64)).cuda(), torch.arange(m, device="cuda")] = 1.0
        XE = torch.empty(m, n, dtype=torch.float64, device="cuda").T
        fn = {"inverse_block": lambda: h.inverse_block(a), "atomic block": lambda: dev.solve_nrhs(a, E, XE), "det block": lambda: dev.solve_nrhs(a, E, XE)}
        res = timed(fn, [("inverse_block", lambda: None), ("atomic block", options(0)), ("det block", options(1))], reps)
        for p, t in res.items():
            print(f"A^-1[S, S], {m} probes: {p:14s} {t[0]:10.3f} ms [{t[1]:.3f}, {t[2]:.3f}]")
    options(0)()
    h.close()


if __name__ == "__main__":
    main()
