"""Host restatement of the forward products with the factor (cholamd_plan_multiply_host): the owner lists of cholamd_multiply_half walked over a host
arena -- no device needed.

Inputs: the four fixtures, a generated 12^3 grid and every synthetic tree of tree_inputs.NAMED + SINGLE, each with row compaction as the environment
leaves it and with CHOLAMD_COMPACT=0 (read at plan creation, hence set in a child process that runs this module's `main`).  The arena holds an
independent factor -- the dense fp64 Cholesky factor of P A P^T, whose structural zeros are exact zeros, as the band and c_lo skips of the leaves
require -- on the stored positions of the lower triangle and NaN everywhere else: the upper triangles of the diagonal blocks and all padding.  A NaN in
y means the walk read something that is not part of the factor.

Gate (multiply_ref): componentwise (k + 2) u |L| |z| against tril(arena_to_dense(arena)) applied in extended precision, k = the most stored entries in a
row (FORWARD) or column (BACKWARD), u = 2^-53: the standard inner-product bound, valid for any summation order.  Nothing is measured."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import multiply_ref as mr
import spd_inputs as si
import tree_inputs
from conftest import CASES, ROOT, case_paths

GENERATED = {"gen_12x12x12": (12, 12, 12, 4, 16)}
TREE_NAMES = tree_inputs.NAMED + tree_inputs.SINGLE
NAMES = list(CASES) + list(GENERATED) + TREE_NAMES


def load_plan(name, tmp):
    import cholesky_amd as ca
    if name in CASES:
        return ca.Plan(*case_paths(name)[:3])
    if name in GENERATED:
        g = GENERATED[name]
        return ca.Problem(*g[:3], levels=g[3], tile=g[4]).plan()
    spec = tree_inputs.TREES[name]
    return si.SPD(str(tmp), spec, 3000 + spec["seed"], name=name, oracle=False, dense=False).plan


def dense_factor(plan):
    D = plan.arena_to_dense(plan.fill_host())
    return np.linalg.cholesky(np.tril(D) + np.tril(D, -1).T)


def check_input(name, tmp):
    """Both products of one input against the gate; returns the largest error / gate ratio."""
    plan = load_plan(name, tmp)
    arena = mr.arena_from_lower(plan, dense_factor(plan))
    assert np.isnan(arena).any() or plan.n == 1, "the upper triangles and the padding hold NaN"
    D, mask = mr.stored_lower(plan, arena)
    assert np.isfinite(D).all()
    perm = plan.perm
    rng = np.random.default_rng(5)
    z = rng.standard_normal(plan.n)
    worst = 0.0
    for which in (mr.FWD, mr.BWD):
        y = plan.multiply_host(arena, which, z)
        yref, absprod = mr.product(D, perm, z, which)
        r = mr.gate_ratio(y, yref, absprod, mr.longest(mask, which))
        print(f"{name} which={which}: error / gate = {r:.3f} (k = {mr.longest(mask, which)})")
        assert r <= 1.0, (name, which, r)
        worst = max(worst, r)
    # in place: the same bits
    w = z.copy()
    assert plan.L.cholamd_plan_multiply_host(plan.h, arena.ctypes.data, mr.BWD, w.ctypes.data, w.ctypes.data) == 0
    assert np.array_equal(w, plan.multiply_host(arena, mr.BWD, z))
    return worst, plan


@pytest.fixture(autouse=True)
def environment(monkeypatch):
    for v in ("CHOLAMD_COMPACT", "CHOLAMD_SOLVE_NO_BAND"):
        monkeypatch.delenv(v, raising=False)


@pytest.mark.parametrize("name", NAMES)
def test_host_multiply_matches_the_dense_image(name, tmp_path):
    check_input(name, tmp_path)


def test_host_multiply_without_row_compaction():
    """CHOLAMD_COMPACT=0 is read when a plan is made: every input again in a child process."""
    env = dict(os.environ, CHOLAMD_COMPACT="0")
    env.pop("CHOLAMD_SOLVE_NO_BAND", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count(" which=") == 2 * len(NAMES) and "uncompacted: ok" in p.stdout


def test_garbage_in_the_upper_triangles_does_not_reach_y(tmp_path):
    """The same arena with zeros and with NaN above the diagonals of the diagonal blocks: the same bits."""
    for name in ("lapl_400x400", "tree_over"):
        plan = load_plan(name, tmp_path)
        L = dense_factor(plan)
        clean, dirty = mr.arena_from_lower(plan, L, fill=0.0), mr.arena_from_lower(plan, L, fill=0.0)
        img = mr.index_image(plan)
        i, j = np.nonzero(np.triu(img, 1))
        assert len(i) > 0, "the diagonal blocks store their upper triangles"
        dirty[img[i, j] - 1] = np.nan
        z = np.random.default_rng(6).standard_normal(plan.n)
        for which in (mr.FWD, mr.BWD):
            a, b = plan.multiply_host(clean, which, z), plan.multiply_host(dirty, which, z)
            assert np.isfinite(b).all() and np.array_equal(a, b), (name, which)


def test_band_skips_change_nothing(tmp_path, monkeypatch):
    """With CHOLAMD_SOLVE_NO_BAND=1 the lists read the structural zeros of the leaves too: the skipped entries are exact zeros, so every
    component stays inside the gate against the same reference (the bits may differ: a sum has more, zero, terms)."""
    plan = load_plan("tree_skew", tmp_path)
    arena = mr.arena_from_lower(plan, dense_factor(plan))
    z = np.random.default_rng(8).standard_normal(plan.n)
    D, mask = mr.stored_lower(plan, arena)
    monkeypatch.setenv("CHOLAMD_SOLVE_NO_BAND", "1")
    for which in (mr.FWD, mr.BWD):
        yref, absprod = mr.product(D, plan.perm, z, which)
        assert mr.gate_ratio(plan.multiply_host(arena, which, z), yref, absprod, mr.longest(mask, which)) <= 1.0


def test_list_sizes(tmp_path):
    """multiply_counts: one item per 16 positions of every separator in both directions; a product reads every non-zero of the factor and nothing
    but stored positions of the lower triangle."""
    for name in ("lapl_3375x3375", "tree_skew"):
        plan = load_plan(name, tmp_path)
        c = plan.multiply_counts()
        items = int(sum((int(m) + 15) // 16 for m in plan.sep_sizes))
        D, mask = mr.stored_lower(plan, mr.arena_from_lower(plan, dense_factor(plan)))
        for w in ("forward", "backward"):
            assert c[w]["items"] == items and c[w]["sources"] >= items
            assert int((D != 0).sum()) <= c[w]["entries"] <= int(mask.sum()), (name, w, c[w])
    assert plan.L.cholamd_plan_multiply_counts(plan.h, None) == -4 and plan.L.cholamd_plan_multiply_counts(None, None) == -4


def test_bad_arguments_are_refused(tmp_path):
    plan = load_plan("lapl_9x9", tmp_path)
    arena = mr.arena_from_lower(plan, dense_factor(plan), fill=0.0)
    z, y = np.ones(plan.n), np.full(plan.n, -7.0)
    f = plan.L.cholamd_plan_multiply_host
    for which in (2, -1):
        assert f(plan.h, arena.ctypes.data, which, z.ctypes.data, y.ctypes.data) == -4
        assert "which" in plan.L.cholamd_last_error().decode()
    assert f(plan.h, None, 0, z.ctypes.data, y.ctypes.data) == -4
    assert f(plan.h, arena.ctypes.data, 0, None, y.ctypes.data) == -4
    assert f(plan.h, arena.ctypes.data, 0, z.ctypes.data, None) == -4
    assert f(None, arena.ctypes.data, 0, z.ctypes.data, y.ctypes.data) == -4
    assert (y == -7.0).all()


def main():
    sys.path.insert(0, ROOT)
    worst = 0.0
    with tempfile.TemporaryDirectory() as tmp:
        for name in NAMES:
            r, plan = check_input(name, tmp)
            if os.environ.get("CHOLAMD_COMPACT") == "0":
                assert plan.arena_doubles == plan.arena_dense_doubles, "row compaction is off"
            worst = max(worst, r)
    print(f"uncompacted: ok, largest error / gate = {worst:.3f}")


if __name__ == "__main__":
    main()
