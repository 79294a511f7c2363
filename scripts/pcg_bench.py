"""Preconditioned CG with the factor at hand against a solve and against a refactorisation (development aid; bench.py is the contract).

python scripts/pcg_bench.py CASE PRECISION NRHS [rounds]
  CASE = a fixture under tests/golden (lapl_3375x3375) or gen:N:LEVELS (the generated N^3 Laplacian, tile 32); PRECISION = fp64 | fp32 (the arena that
  holds the factor of A); NRHS = columns.  A' = A + 0.1 diag(a_ii xi_i), xi uniform in [0, 1], is applied by set_values; the arena keeps the factor of A.
  HIP events on one stream; every variant runs once per round, in turn; one JSON line with median [min, max] in ms:
    solve        one cholamd_solve / _nrhs (_f32) call with the factor of A
    pcg          cholamd_solve_pcg / _nrhs (_f32) on A' to 1e-12: the whole call, its iteration count, ms per iteration
    values_pcg   set_values(A') + pcg
    refactor     set_values(A') + fill + factor + solve
    apply        cholamd_apply / _nrhs alone, with the bytes it has to move (CSR once per 8 columns, p and q once per column) over its time"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import cholesky_amd as ca

case, prec, nrhs = sys.argv[1], sys.argv[2], int(sys.argv[3])
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 7
assert prec in ("fp64", "fp32"), prec
if case.startswith("gen:"):
    _, N, lv = case.split(":")
    plan = ca.Problem(int(N), int(N), int(N), int(lv), 32).plan()
    r, c = plan.entries()
    v0 = np.where(r == c, 6.0, -1.0)  # the generator's 7-point Laplacian
else:
    G = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", case)
    files = sorted(os.listdir(G))
    mtx = os.path.join(G, [f for f in files if f.startswith("lapl") and f.endswith(".mtx")][0])
    plan = ca.Plan(mtx, os.path.join(G, [f for f in files if "_ord_" in f][0]), os.path.join(G, [f for f in files if "_clust_" in f][0]))
    r, c = plan.entries()
    v0 = np.ascontiguousarray(np.loadtxt(mtx, comments="%")[1:, 2])
n = plan.n
probe = np.random.default_rng(0).standard_normal(n)
assert np.array_equal(plan.apply_host(probe), plan.apply_host(probe, values=v0)), "the value array is not the plan's"
v1 = v0.copy()
dg = r == c
v1[dg] *= 1.0 + 0.1 * np.random.default_rng(11).uniform(0.0, 1.0, int(dg.sum()))
dev = ca.Device(plan, 0)
f32 = prec == "fp32"
arena = dev.new_arena_f32() if f32 else dev.new_arena()
arena2 = dev.new_arena_f32() if f32 else dev.new_arena()  # the refactorisation's
fill, factor = (dev.fill_f32, dev.factor_f32) if f32 else (dev.fill, dev.factor)
fill(arena)
factor(arena)
dev.sync()
assert dev.info() == (0, 0), dev.info()
d_v0, d_v1 = torch.from_numpy(v0).cuda(), torch.from_numpy(v1).cuda()
g = torch.Generator(device="cuda").manual_seed(1)
B = torch.randn(nrhs, n, dtype=torch.float64, device="cuda", generator=g).T
X = torch.zeros(nrhs, n, dtype=torch.float64, device="cuda").T
Y = torch.zeros(nrhs, n, dtype=torch.float64, device="cuda").T
its = []


def solve(a=arena):
    if nrhs == 1:
        (dev.solve_f32 if f32 else dev.solve)(a, B[:, 0], X[:, 0])
    else:
        dev.solve_nrhs(a, B, X)


def pcg():
    if nrhs == 1:
        it, rel, st = dev.solve_pcg(arena, B[:, 0], X[:, 0], max_iter=100, tol=1e-12)
        it, st = np.array([it]), np.array([st])
    else:
        it, rel, st = dev.solve_pcg_nrhs(arena, B, X, max_iter=100, tol=1e-12)
    assert (st == 0).all(), (it, rel, st)
    its.append(int(it.max()))


def values_pcg():
    dev.set_values(d_v1, check=False)
    pcg()


def refactor():
    dev.set_values(d_v1, check=False)
    fill(arena2)
    factor(arena2)
    solve(arena2)


def apply():
    if nrhs == 1:
        dev.apply(B[:, 0], Y[:, 0])
    else:
        dev.apply_nrhs(B, Y)


variants = dict(solve=solve, pcg=pcg, values_pcg=values_pcg, refactor=refactor, apply=apply)
dev.set_values(d_v1)
for fn in variants.values():  # warm-up: every workspace and list exists
    fn()
dev.sync()
ms = {k: [] for k in variants}
for _ in range(rounds):
    for k, fn in variants.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms[k].append(e0.elapsed_time(e1))
assert dev.info() == (0, 0), dev.info()


def stat(v):
    return [round(float(np.median(v)), 4), round(float(min(v)), 4), round(float(max(v)), 4)]


nnz = int(dg.sum()) + 2 * int((~dg & (v0 != 0)).sum())
apply_bytes = ((nrhs + 7) // 8 if nrhs > 1 else 1) * (12 * nnz + 8 * (n + 1)) + nrhs * 16 * n
it = int(np.median(its))
out = dict(case=case, precision=prec, nrhs=nrhs, n=n, rounds=rounds, iterations=it, ms={k: stat(v) for k, v in ms.items()},
           pcg_ms_per_iteration=round(float(np.median(ms["pcg"])) / max(it, 1), 4),
           pcg_iteration_over_solve=round(float(np.median(ms["pcg"])) / max(it, 1) / float(np.median(ms["solve"])), 3),
           refactor_over_values_pcg=round(float(np.median(ms["refactor"])) / float(np.median(ms["values_pcg"])), 2),
           apply_bytes=apply_bytes, apply_TBps=round(apply_bytes / (float(np.median(ms["apply"])) * 1e-3) / 1e12, 3))
print(json.dumps(out))
