"""The place of a follower's own tiles in the one-launch factor (option follow_own; tests/follow_own_inputs.py trees, CHOLAMD_POISON=1).

A POTRF job that follows its sources starts from zero accumulators, subtracts the followed column tiles as they arrive and adds its own tiles --
A's entries plus what update jobs have brought -- at a place the schedule fixes per job (chol_job.mode): in front of the round of its last two
items (follow_own 0, and every follower whose own tiles are ready early), or after the last item (follow_own 1, the default: where early update
jobs write the follower's diagonal block; follow_own 2: every follower with waits).  The place is a position in the floating-point sum, so the
factors of the three values differ by rounding, and each of them must be the same bits in every run.

Every case takes the default (program-launch) path -- program_trace raises where there is none -- and is held to the factor checks of
tests/test_gpu_trees.py: info (0, 0), the oracle's zero pattern entry for entry, row error and reconstruction within spd_inputs' tolerances;
the oracle's own factor of the input is held to the same tolerances first.  Two factorisations on one device object and one on a fresh device
object give the same bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import follow_own_inputs as fi  # noqa: E402
import spd_inputs as si  # noqa: E402
from test_gpu_poison import _factor  # noqa: E402
from test_gpu_trees import _check_factor, _device  # noqa: E402


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("CHOLAMD_POISON", "1")


@pytest.fixture(scope="module", params=fi.NAMES)
def case(request, tmp_path_factory):
    """(name, input with the oracle's factor): built once per spec, shared by the three follow_own values, never written to."""
    name = request.param
    S = si.cached(tmp_path_factory, "own_" + name, build=lambda tmp_path: fi.spd(tmp_path, name))
    # the input carries the check: the oracle's own factor meets the tolerances the helper applies (tests/test_tree_inputs.py)
    assert S.row_error(S.Lo) <= S.tol_factor() and S.reconstruction(S.Lo) <= S.tol_reconstruction() and not S.Lo[S.Ld == 0].any()
    return name, S


@pytest.mark.parametrize("follow_own", fi.FOLLOW_OWN)
def test_follow_own(case, follow_own):
    name, S = case
    what = f"{name} follow_own={follow_own}"
    P = S.plan
    # the place the kernel will take is the one the host reports for this option: followers with waits exist, and the option moves them
    fol = P.program_follow_own(follow_own)
    waits = [f for f in fol if f["n_wait"] > 0]
    assert waits, what
    if follow_own == 0:
        assert all(f["own_at"] < f["n_ext"] for f in fol), what
    else:
        assert any(f["own_at"] == f["n_ext"] for f in waits), what
    dev = _device(P, {"follow_own": follow_own})
    a = _factor(dev)                                                   # guarded arena; info == (0, 0); guards intact
    assert dev.info() == (0, 0)
    _check_factor(S, a, False, what)
    first = a.t.cpu().numpy().copy()
    dev.fill(a.t)
    dev.factor(a.t)
    dev.sync()
    assert dev.info() == (0, 0)
    a.assert_guards("arena")
    assert np.array_equal(first, a.t.cpu().numpy()), what + ": second factorisation on the same device object"
    dev.fill(a.t)
    assert len(dev.program_trace(a.t)) > 0                             # the program launch was taken (raises otherwise) ...
    dev.sync()
    assert dev.info() == (0, 0)
    _check_factor(S, a, False, what + " (trace build)")               # ... and its diagnostic instance computes the same factor
    assert np.array_equal(first, a.t.cpu().numpy()), what + ": trace build"
    dev2 = _device(P, {"follow_own": follow_own})
    b = _factor(dev2)
    assert dev2.info() == (0, 0)
    assert np.array_equal(first, b.t.cpu().numpy()), what + ": fresh device object"
