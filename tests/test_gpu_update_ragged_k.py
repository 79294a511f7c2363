"""Extend-add tasks of the one-launch factor on sources of ragged width (tests/tree_inputs.py trees, CHOLAMD_POISON=1).

An update task of the program launch reads its sources -- the solved strips of a descendant separator of K columns -- in batches of up to 32
columns (8 MFMA k-steps of 4 columns), two batches per memory round trip; the last batch of a source is partial (1 .. 8 k-steps, the last k-step
of K mod 4 columns) and the next source's first batch rides along with it.  The separator of s columns is the source: as a leaf (its tasks go into
the parent and the root) and as the middle separator (into the root, next to the sources of its own children).

  light tasks (one wave a task): s covers every k-step count 1 .. 8 of a partial batch (2 3 5 7 9 13 18 19 22 27 29 30 -> 1 1 2 2 3 4 5 5 6 7 8 8),
    K mod 4 = 1, 2, 3, K < 32, one full batch and a partial one (35 39 41 45 51 59), several full batches and a partial one (70 98 101 115), and
    the 39 / 51 / 98 of lapl_3375x3375
  heavy tasks (>= 48 k-steps, K split four ways over the waves of a group): ("band", 17) leaves of 193 .. 270 columns, factored unsplit
  "tiles" couplings: range-masked cells (chol_upd_src.range) through the partial batch

Every case takes the default (program-launch) path -- program_trace raises where there is none -- and is held to the factor checks of
tests/test_gpu_trees.py: info (0, 0), the oracle's zero pattern entry for entry, row error and reconstruction within spd_inputs' tolerances."""
import pytest

pytestmark = pytest.mark.gpu

import spd_inputs as si  # noqa: E402
import tree_inputs as ti  # noqa: E402
from test_gpu_poison import _factor  # noqa: E402
from test_gpu_trees import _check_factor, _device  # noqa: E402

LIGHT = [2, 3, 5, 7, 9, 13, 18, 19, 22, 27, 29, 30, 35, 39, 41, 45, 51, 59, 70, 98, 101, 115]
HEAVY = [193, 201, 219, 237, 255, 259, 270]
assert sorted({(s % 32 + 3) // 4 for s in LIGHT if s % 32}) == list(range(1, 9)) and {s % 4 for s in LIGHT} == {1, 2, 3}


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("CHOLAMD_POISON", "1")


def _run(tmp_path, spec, heap, s, name):
    S = si.SPD(str(tmp_path), spec, 3000 + spec["seed"], name=name)
    P = S.plan
    assert P.sep_sizes[P.tree[heap - 1] - 1] == s and P.levels == 3
    dev = _device(P, {})
    a = _factor(dev)                                                   # guarded arena; info == (0, 0); guards intact
    assert dev.info() == (0, 0)
    _check_factor(S, a, False, name)
    dev.fill(a.t)
    assert len(dev.program_trace(a.t)) > 0                             # the program launch was taken (raises otherwise) ...
    dev.sync()
    assert dev.info() == (0, 0)
    _check_factor(S, a, False, name + " (trace build)")               # ... and its diagnostic instance computes the same factor


@pytest.mark.parametrize("s", LIGHT)
@pytest.mark.parametrize("position", ["leaf", "middle"])
def test_light_tasks(position, s, tmp_path):
    _run(tmp_path, ti.sweep_spec(position, s), {"leaf": 4, "middle": 2}[position], s, f"ragged_{position}_{s}")


@pytest.mark.parametrize("s", HEAVY)
def test_heavy_tasks(s, tmp_path):
    _run(tmp_path, ti.sweep_spec("leaf", s, ("band", 17)), 4, s, f"ragged_band17_{s}")


@pytest.mark.parametrize("position,s", [("leaf", 39), ("middle", 51)])
def test_tiles_coupling(position, s, tmp_path):
    spec = dict(ti.sweep_spec(position, s), coupling=["tiles"])
    _run(tmp_path, spec, {"leaf": 4, "middle": 2}[position], s, f"ragged_tiles_{position}_{s}")
