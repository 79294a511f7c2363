"""Refactorisation with new values of A: Device.set_values against a new plan (development aid; bench.py is the contract).

python scripts/refactor_bench.py CASE [fp64|fp32] [--reps R] [--warmup W] [--new-plan-reps C] [--parts abcd] [--package-root DIR]
  CASE = a fixture under tests/golden, or gen:N:levels (an N^3 Laplacian, tile 64: bench.py's large fronts).  The matrix is read into arrays
  once (untimed) and the plan under test is Plan.from_arrays of them, so that the value array is simply the array of values.  Two value sets
  of one pattern (A and 1.5 A) alternate between repeats.  Parts:
    a  set_values alone, checked (one synchronisation, 32 bytes read back) and unchecked (asynchronous)
    b  set_values + fill + factor, checked and unchecked
    c  what a library without set_values offers for new values: Plan.from_arrays + Device + fill + factor (host clock, device synchronised)
    d  fill + factor alone
  a, b, d: one stream, an event pair per repeat after `warmup` untimed repeats; min / median / max of the repeats in ms, and the host's wall
  time per repeat of the whole loop (what a caller that waits for each step sees).  --package-root imports cholesky_amd from another checkout
  (parts c and d exist on commits without set_values: time them there in the same session).  Prints one JSON line, with the byte count of the
  gather: 8 nz read at random, (8 + 4) (nnz_a + csr) streamed, and 9 nz for the status words."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("case", nargs="?", default="lapl_3375x3375")
ap.add_argument("precision", nargs="?", default="fp64", choices=("fp64", "fp32"))
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--new-plan-reps", type=int, default=3)
ap.add_argument("--parts", default="abcd")
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, args.package_root)
import numpy as np
import torch

import cholesky_amd as ca
from cholesky_amd._lib import SepInfo, check, load

L = load()
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
with tempfile.TemporaryDirectory() as tmp:
    if args.case.startswith("gen:"):
        _, N, lv = args.case.split(":")
        mtx, ordf, clf, _ = ca.Problem(int(N), int(N), int(N), int(lv), 64).write(os.path.join(tmp, "gen"))
    else:
        G = os.path.join(GOLDEN, args.case)
        files = sorted(os.listdir(G))
        mtx, ordf, clf = (os.path.join(G, [f for f in files if pick(f)][0]) for pick in
                          (lambda f: f.startswith("lapl") and f.endswith(".mtx"), lambda f: "_ord_" in f, lambda f: "_clust_" in f))
    with open(mtx) as f:
        banner = f.readline().strip()
        n, _, nz = (int(v) for v in f.readline().split())
    perm, sep = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    info = SepInfo()
    check(L.cholamd_read_separators(os.fsencode(ordf), n, perm.ctypes.data, sep.ctypes.data, C.byref(info)), "read_separators")
    assert (np.diff(sep) >= 0).all(), "from_arrays takes the separators in label order"
    sep_sizes = np.bincount(sep, minlength=info.num_separators + 1)[1:].astype(np.int32)
    cnt = C.c_int64(0)
    assert L.cholamd_read_clusters(os.fsencode(clf), None, None, None, 0, C.byref(cnt)) >= 0
    cl = [np.zeros(cnt.value + 1, dtype=np.int32) for _ in range(3)]
    assert L.cholamd_read_clusters(os.fsencode(clf), cl[0].ctypes.data, cl[1].ctypes.data, cl[2].ctypes.data, cnt.value, C.byref(cnt)) >= 0
    cl = [a[:cnt.value] for a in cl]
    row, col, val = np.zeros(nz, dtype=np.int32), np.zeros(nz, dtype=np.int32), np.zeros(nz, dtype=np.float64)
    check(L.cholamd_read_matrix(os.fsencode(mtx), nz, row.ctypes.data, col.ctypes.data, val.ctypes.data), "read_matrix")


def new_plan(v):
    return ca.Plan.from_arrays(n, info.levels, perm, sep_sizes, cl[0], cl[1], cl[2], row, col, v, banner=banner)


f32 = args.precision == "fp32"
vals = [val, 1.5 * val]
plan = new_plan(vals[0])
dev = ca.Device(plan, 0)
arena = dev.new_arena_f32() if f32 else dev.new_arena()
stream = torch.cuda.current_stream()


def fill_factor(d=dev, a=arena):
    (d.fill_f32 if f32 else d.fill)(a, stream=stream)
    (d.factor_f32 if f32 else d.factor)(a, stream=stream)


def timed(fn):
    """fn(i) `warmup` times untimed, then `reps` times between event pairs on the stream."""
    for i in range(args.warmup):
        fn(i)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
    t0 = time.perf_counter()
    for i, (a, b) in enumerate(ev):
        a.record(stream)
        fn(i)
        b.record(stream)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / args.reps
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    assert dev.info() == (0, 0), dev.info()
    return dict(min=round(ms[0], 4), median=round(ms[len(ms) // 2], 4), max=round(ms[-1], 4), wall_per_rep=round(wall, 4))


ncsr = 2 * plan.nnz_a - n  # both triangles (none of these cases has dropped entries or explicit zeros)
out = dict(case=args.case, precision=args.precision, n=n, nz=int(nz), nnz_a=int(plan.nnz_a), arena_GB=round(plan.arena_doubles * (4 if f32 else 8) / 1e9, 3),
           reps=args.reps, warmup=args.warmup, package_root=args.package_root, ms={})
if "a" in args.parts or "b" in args.parts:
    dvals = [torch.from_numpy(v).cuda() for v in vals]
    out["gather_bytes"] = dict(random=8 * int(nz), streamed=12 * int(plan.nnz_a + ncsr), status=9 * int(nz))
if "d" in args.parts:
    out["ms"]["d_fill_factor"] = timed(lambda i: fill_factor())
if "a" in args.parts:
    out["ms"]["a_set_values_checked"] = timed(lambda i: dev.set_values(dvals[i & 1], check=True, stream=stream))
    out["ms"]["a_set_values_unchecked"] = timed(lambda i: dev.set_values(dvals[i & 1], check=False, stream=stream))
if "b" in args.parts:
    for name, chk in (("b_set_values_fill_factor_checked", True), ("b_set_values_fill_factor_unchecked", False)):
        out["ms"][name] = timed(lambda i: (dev.set_values(dvals[i & 1], check=chk, stream=stream), fill_factor()))
if "d" in args.parts:  # once more: the spread of (d) between two places of one process
    out["ms"]["d_fill_factor_again"] = timed(lambda i: fill_factor())
if "c" in args.parts:
    ts = []
    for i in range(args.new_plan_reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p2 = new_plan(vals[i & 1])
        t1 = time.perf_counter()
        d2 = ca.Device(p2, 0)
        t2 = time.perf_counter()
        fill_factor(d2, arena)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        assert d2.info() == (0, 0), d2.info()
        ts.append(((t3 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
        del d2, p2
    ts = sorted(ts[1:])  # the first one is the warm-up
    out["ms"]["c_new_plan_device_fill_factor"] = dict(zip(("total", "plan", "device", "fill_factor"), (round(v, 3) for v in ts[len(ts) // 2])), min_total=round(ts[0][0], 3),
                                                      max_total=round(ts[-1][0], 3), reps=args.new_plan_reps)
print(json.dumps(out))
