"""Host side of the followers' own tiles (option follow_own) and of the update jobs' write order -- no GPU.

The schedule fixes, per following POTRF job, the followed item in front of whose round the job adds its own tiles (chol_job.mode; the number of
items = after the last one); the kernel takes it from the job.  Plan.program_follow_own reports it under given options, Plan.program_check_opts
simulates the queue (and refuses a place that is not the start of a round), Plan.program_hazards works out from the counters' meaning whether
any two update jobs that write a common arena element are ordered."""
import ctypes as C

import pytest

import follow_own_inputs as fi
from conftest import case_paths

FIXTURES = ["lapl_25x25", "lapl_400x400", "lapl_3375x3375"]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    import cholesky_amd as ca
    tmp = tmp_path_factory.mktemp("follow_own_host")
    out = {name: fi.spd(tmp, name, oracle=False).plan for name in fi.NAMES}
    out.update({case: ca.Plan(*case_paths(case)[:3]) for case in FIXTURES})
    return out


def _rounds(n_ext, T):
    from cholesky_amd import _lib
    buf = (C.c_int * 64)()
    own = C.c_int(-1)
    n = _lib.load().cholamd_follow_rounds(n_ext, T, 64, buf, C.byref(own))
    return [buf[i] for i in range(n)], own.value


def test_the_cases_hold_every_kind_of_follower(plans):
    """Under the default option the trees hold a follower with its own tiles last, one with waits at the default place and one without waits;
    lists of pair rounds and of single rounds, of odd and of even length; every place is the start of a round or the end of the list."""
    kinds, rounds, parity = set(), set(), set()
    for name in fi.NAMES:
        fol = plans[name].program_follow_own()
        assert fol == plans[name].program_follow_own(1), name                           # the default is 1
        for f in fol:
            r, own = _rounds(f["n_ext"], f["T"])
            starts = [sum(r[:i]) for i in range(len(r))] + [f["n_ext"]]
            assert f["own_at"] in starts, (name, f)
            kinds.add("none" if f["n_wait"] == 0 else "last" if f["own_at"] == f["n_ext"] else "default")
            if f["n_wait"] == 0 or f["own_at"] < f["n_ext"]:
                assert f["own_at"] == own, (name, f)                                      # the default place: chol_follow_own_at
            rounds |= set(r)
            parity.add(f["n_ext"] % 2)
            if f["n_wait"] > 0 and f["own_at"] == f["n_ext"]:
                assert f["T"] > 4, (name, f)                                              # only wide followers have early update jobs
    assert kinds == {"none", "last", "default"} and rounds == {1, 2} and parity == {0, 1}, (kinds, rounds, parity)


def test_follow_own_0_is_the_default_place_everywhere(plans):
    """follow_own = 0 reproduces chol_follow_own_at for every follower of the fixtures (and of the trees); 2 moves every follower with waits to the
    end and nobody else; 1 moves a subset of those; items, tile columns and waits do not depend on the option."""
    for name, P in plans.items():
        f0, f1, f2 = (P.program_follow_own(v) for v in (0, 1, 2))
        key = lambda fol: [(f["job"], f["n_ext"], f["T"], f["n_wait"]) for f in fol]      # noqa: E731
        assert key(f0) == key(f1) == key(f2) and len(f0) > 0, name
        for a, b, c in zip(f0, f1, f2):
            assert a["own_at"] == _rounds(a["n_ext"], a["T"])[1], (name, a)
            assert c["own_at"] == (c["n_ext"] if c["n_wait"] > 0 else a["own_at"]), (name, c)
            assert b["own_at"] in (a["own_at"], c["own_at"]), (name, b)
    # the flagship case: the wide followers of the pivot chain (two separators under the root, the root's two column blocks) and nobody else
    moved = [(f["n_ext"], f["T"]) for f in plans["lapl_3375x3375"].program_follow_own(1) if f["own_at"] == f["n_ext"] and f["n_wait"] > 0]
    assert sorted(moved) == [(3, 7), (6, 7), (6, 7), (6, 8)], moved
    assert plans["lapl_400x400"].program_follow_own(1) == plans["lapl_400x400"].program_follow_own(0)


@pytest.mark.parametrize("follow_own", fi.FOLLOW_OWN)
def test_the_queue_stays_live(plans, follow_own):
    """program_check_opts passes for the fixtures and the trees under every follow_own value, also under follow_tail 0 / 1 / 3 / 7 and with 16, 64 and
    256 resident workgroups."""
    for name, P in plans.items():
        P.program_check_opts(follow_own=follow_own)
        for tail in (0, 1, 3, 7):
            for workers in (16, 64, 256):
                P.program_check_opts(follow_tail=tail, follow_own=follow_own, workers=workers)


def test_update_jobs_that_share_a_tile_are_ordered(plans):
    """Any two update jobs that write a common arena element are ordered through the later one's gating waits, transitively: the later job cannot start
    before the earlier one has completed, whatever the timing.  (A wait counts arrivals: what it guarantees depends on who else raises the counter
    and what THEY wait for.  Update jobs into a diagonal block that waited for the diagonal block's counter alone would raise the panel's counter
    early and let an update job of the next phase into another block of the panel start over an unfinished one: this check refuses that schedule.)"""
    shared = 0
    for name, P in plans.items():
        for opts in ({}, {"follow_own": 0}, {"follow_own": 2}, {"follow_tail": 1}, {"follow_tail": 0}, {"split_min": 64, "split_nb": 64, "follow_tail": 1},
                     {"split_min": 96, "split_nb": 96}):
            pairs, unordered, first = P.program_hazards(**opts)
            assert unordered == 0 and first == (-1, -1), (name, opts, pairs, unordered, first)
            shared += pairs
    assert shared > 0
