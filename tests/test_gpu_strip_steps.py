"""TRSM strips of the one-launch factor: the flag-synchronised step loop (tests/tree_inputs.py trees, CHOLAMD_POISON=1).

In the program launch a strip of 16 rows below a pivot block is solved column tile by column tile by four waves (trsm_rr_body); the owner of
tile J + 1 (wave (J + 1) mod 4) brings it up to date with X_J, solves it, writes X_{J+1} to an LDS slot of its own and sets that tile's flag; the
other waves wait for the flag, not for a workgroup barrier, and the three strips of a job run independently of each other.  The separator of s
columns is the pivot whose strips are followed by its parent: as a leaf (followed by the middle separator) and as the middle separator
(followed by the root).

  s = 1 15 16 17 32 33 48 49 64 65: 1 .. 5 column tiles -- no look-ahead at all, the owner rotation up to its first wrap (tile 4 is wave 0's
    second), a ragged last tile next to a full one
  s = 80 81 128 129 176: two and three tiles per wave; 176 is the widest dense pivot the program launch keeps whole
  s = 177: a split pivot (96 + 81), whose second block follows the strips of the first
  ("band", 17) leaves of 193, 259 and 272 columns: the band form, 13 .. 17 column tiles, up to five per wave

The fixed neighbour sizes of sweep_spec (5, 17, 33, 37 rows) give strips of 1 and 5 valid rows and jobs of one, two and three strips (the groups
of a job without a strip leave at once): test_the_plans_hold_the_strip_cases reads that from the plans.

Every case takes the default (program-launch) path -- program_trace raises where there is none -- and is held to the factor checks of
tests/test_gpu_trees.py: info (0, 0), the oracle's zero pattern entry for entry, row error and reconstruction within spd_inputs' tolerances;
the oracle's own factor of the input is held to the same tolerances first."""
import pytest

pytestmark = pytest.mark.gpu

import spd_inputs as si  # noqa: E402
import tree_inputs as ti  # noqa: E402
from test_gpu_poison import _factor  # noqa: E402
from test_gpu_trees import _check_factor, _device  # noqa: E402

FEW_TILES = [1, 15, 16, 17, 32, 33, 48, 49, 64, 65]
MANY_TILES = [80, 81, 128, 129, 176]
SPLIT = [177]
BAND = [193, 259, 272]
HEAP = {"leaf": 4, "middle": 2}
CASES = [(pos, s, "dense") for pos in ("leaf", "middle") for s in FEW_TILES + MANY_TILES + SPLIT] + [("leaf", s, ("band", 17)) for s in BAND]
assert sorted({(s + 15) // 16 for s in FEW_TILES}) == [1, 2, 3, 4, 5] and {(s + 15) // 16 for s in BAND} == {13, 17}


def _id(case):
    pos, s, leaf = case
    return f"{pos}_{s}" if leaf == "dense" else f"{pos}_band{leaf[1]}_{s}"


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("CHOLAMD_POISON", "1")


def _strip_jobs(P):
    """(strips, pivot label, channel) of every strip job of the plan's program."""
    jobs, _ = P.program_jobs()
    return [(int(j[4]), int(j[1]), int(j[6])) for j in jobs if j[0] == 1]


def _strip_rows(P):
    """Valid rows of every 16-row strip the plan stores below a pivot."""
    rows = set()
    for b in P.blocks:
        r, c = int(b[0]), int(b[1])
        if r != c:
            m = int(P.sep_sizes[r - 1])
            rows |= {min(16, m - 16 * t) for t, at in enumerate(P.block_tile_map(r, c)) if at >= 0 and 16 * t < m}
    return rows


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_strip_steps(case, tmp_path):
    pos, s, leaf = case
    name = "strips_" + _id(case)
    spec = ti.sweep_spec(pos, s, leaf)
    S = si.SPD(str(tmp_path), spec, 3000 + spec["seed"], name=name)
    P = S.plan
    lbl = int(P.tree[HEAP[pos] - 1])
    assert P.sep_sizes[lbl - 1] == s and P.levels == 3
    # the input carries the check: the oracle's own factor meets the tolerances the helper applies (tests/test_tree_inputs.py)
    assert S.row_error(S.Lo) <= S.tol_factor() and S.reconstruction(S.Lo) <= S.tol_reconstruction() and not S.Lo[S.Ld == 0].any()
    # the pivot's strips are there, and a parent follows them (a channel)
    mine = [j for j in _strip_jobs(P) if j[1] == lbl]
    assert mine and all(1 <= n <= 3 for n, _, _ in mine) and any(chan >= 0 for _, _, chan in mine), mine
    dev = _device(P, {})
    a = _factor(dev)                                                   # guarded arena; info == (0, 0); guards intact
    assert dev.info() == (0, 0)
    _check_factor(S, a, False, name)
    dev.fill(a.t)
    assert len(dev.program_trace(a.t)) > 0                             # the program launch was taken (raises otherwise) ...
    dev.sync()
    assert dev.info() == (0, 0)
    _check_factor(S, a, False, name + " (trace build)")               # ... and its diagnostic instance computes the same factor


def test_the_plans_hold_the_strip_cases(tmp_path):
    """Read from the plans of the cases (no oracle, no device): strip jobs of one, two and three strips, strips of 1, 5 and 16 valid rows, and a
    split 177 whose first block's strips have a channel of their own."""
    counts, rows = set(), set()
    for pos, s, leaf in [c for c in CASES if c[1] in (1, 17, 177, 272)]:
        P = ti.sweep(tmp_path, pos, s, leaf, oracle=False).plan
        jobs = _strip_jobs(P)
        counts |= {n for n, _, _ in jobs}
        rows |= _strip_rows(P)
        if s == 177:
            lbl = int(P.tree[HEAP[pos] - 1])
            assert len({chan for _, sep, chan in jobs if sep == lbl and chan >= 0}) >= 2, jobs
    assert counts == {1, 2, 3}, counts
    assert {1, 5, 16} <= rows, rows
