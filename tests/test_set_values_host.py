"""The value array on the host: Plan.entries(), Plan.value_map() and Plan.fill_host(values=...) -- the plan remembers where every entry of the
list it was created from went, so that new values on the same pattern can be scattered without a new plan (the device side:
test_gpu_set_values.py).  Every comparison is against a second plan created from the same entries with the new values."""
import os

import numpy as np
import pytest

import spd_inputs as si
from conftest import CASES, case_paths

GRIDS = {"g12_full": ((12, 12, 12, 4, 16), {"pattern": "full"}), "g10_own": ((10, 10, 10, 3, 16), {"pattern": "own"})}


def read_mtx(path):
    """(banner, n, row, col, val) of a coordinate file, entries 0-based in file order."""
    with open(path) as f:
        banner = f.readline().rstrip("\n")
        line = f.readline()
        while line.startswith("%"):
            line = f.readline()
        n, _, nz = (int(v) for v in line.split())
        d = np.loadtxt(f, ndmin=2)
    assert len(d) == nz
    return banner, n, d[:, 0].astype(np.int64) - 1, d[:, 1].astype(np.int64) - 1, d[:, 2].copy()


def write_like(path, banner, n, row, col, val):
    """The same entries in the same order with other values (%.17g: fp64 round-trips exactly)."""
    with open(path, "w") as f:
        f.write("%s\n%d %d %d\n" % (banner, n, n, len(val)))
        f.writelines("%d %d %.17g\n" % (row[e] + 1, col[e] + 1, val[e]) for e in range(len(val)))


def values_in_order(S, row, col):
    """The values of the SPD input S for the entry list (row, col) (either triangle)."""
    lut = {(int(r), int(c)): v for r, c, v in zip(S.row, S.col, S.val)}
    return np.array([lut[(max(int(r), int(c)), min(int(r), int(c)))] for r, c in zip(row, col)])


def pair(tmp_path, name):
    """(plan 1, the matrix file it was made from, ordering, clusters, S2): plan 1 on a fixture's own file or on a generated input of seed 1,
    S2 = a general SPD input of another seed on the same pattern (its dense P A2 P^T is the independent reference)."""
    import cholesky_amd as ca
    if name in CASES:
        m, o, c, _ = case_paths(name)
        S2 = si.SPD(str(tmp_path), name, 77, oracle=False, name="second")
        return ca.Plan(m, o, c), m, o, c, S2
    base, opts = GRIDS[name]
    S1 = si.SPD(str(tmp_path), base, 5, oracle=False, dense=False, name="first", **opts)
    S2 = si.SPD(str(tmp_path), base, 77, oracle=False, name="second", **opts)
    return S1.plan, S1.mtx, S1.ord, S1.clust, S2


NAMES = list(CASES) + list(GRIDS)


@pytest.mark.parametrize("name", NAMES)
def test_entries_are_the_files_list_and_the_value_map_is_a_bijection(name, tmp_path):
    plan, m, _, _, _ = pair(tmp_path, name)
    _, n, row, col, val = read_mtx(m)
    r, c = plan.entries()
    assert len(r) == plan.nz == len(row)
    assert np.array_equal(r, row) and np.array_equal(c, col)          # file order, original coordinates
    vm = plan.value_map()
    assert len(vm) == plan.nnz_a
    assert len(np.unique(vm)) == len(vm)                               # one scatter entry per entry of the list
    in_pattern = np.nonzero(val != 0.0)[0]
    assert plan.dropped == 0
    assert np.array_equal(np.sort(vm), in_pattern)                     # ... onto the in-pattern entries
    # the scatter list itself: the plan's own fill is its values through the map, at ascending arena offsets
    a = plan.fill_host()
    pos = np.nonzero(a)[0]
    assert len(pos) == len(vm) and np.array_equal(a[pos], val[vm])


@pytest.mark.parametrize("name", NAMES)
def test_fill_host_with_values_is_the_fill_of_a_plan_made_with_them(name, tmp_path):
    import cholesky_amd as ca
    plan, m, o, c, S2 = pair(tmp_path, name)
    banner, n, row, col, v1 = read_mtx(m)
    v2 = values_in_order(S2, row, col)
    assert np.abs(v2 - v1).max() > 0
    m2 = os.path.join(str(tmp_path), "same_order.mtx")
    write_like(m2, banner, n, row, col, v2)
    fresh = ca.Plan(m2, o, c)
    own = plan.fill_host()
    got = plan.fill_host(values=v2)
    assert np.array_equal(got.view(np.uint64), fresh.fill_host().view(np.uint64))      # bit for bit
    P = np.tril(plan.arena_to_dense(got))
    assert np.array_equal(P, np.tril(S2.PAP))                                            # P A2 P^T built in numpy
    assert np.array_equal(plan.fill_host().view(np.uint64), own.view(np.uint64))         # the plan keeps its own values
    assert np.array_equal(plan.fill_host(values=v1).view(np.uint64), own.view(np.uint64))


def test_an_explicit_zero_is_outside_the_pattern_and_wrong_counts_are_refused(tmp_path):
    import cholesky_amd as ca
    from cholesky_amd._lib import CholamdError
    m, o, c, _ = case_paths("lapl_400x400")
    banner, n, row, col, val = read_mtx(m)
    k = int(np.nonzero(row != col)[0][37])
    z = val.copy()
    z[k] = 0.0
    mz = os.path.join(str(tmp_path), "zero.mtx")
    write_like(mz, banner, n, row, col, z)
    plan = ca.Plan(mz, o, c)
    assert plan.nz == len(val) and plan.nnz_a == len(val) - 1
    r, cc = plan.entries()
    assert (r[k], cc[k]) == (row[k], col[k])                           # still in the list ...
    vm = plan.value_map()
    assert k not in set(vm.tolist())                                   # ... with no place in the scatter
    assert np.array_equal(np.sort(vm), np.delete(np.arange(len(val)), k))
    # a value for it is not scattered: the fill with the original values is the fill of the file with the zero
    assert np.array_equal(plan.fill_host(values=val), plan.fill_host())
    for bad in (val[:-1], np.concatenate([val, [1.0]]), val[:0]):
        with pytest.raises(CholamdError, match="value array"):
            plan.fill_host(values=bad)
