"""Level ranges of the level-by-level factorisation (cholamd_factor_levels / cholamd_factor_levels_f32): the driver both precisions share.

A factorisation cut into two calls at any level, the whole range in one call, a range given past both ends and the whole-factor call run the same
launches in the same order on the same schedule, so the arenas are equal BIT FOR BIT (torch.equal) and the pivot status stays (0, 0): the status
words are cleared only by the call whose range starts at the top level, the second call of a cut goes on from the first one's.  fp64 runs with the
program launch off (`program: 0`), with and without the fused launches; the whole-factor call is then the same path.  fp32 runs on its own
schedule, built once per device object at the first fp32 call -- the options are set before it."""
import pytest

from conftest import case_paths

pytestmark = pytest.mark.gpu

PLANS = ["lapl_400x400", "lapl_3375x3375"]
FP64_OPTIONS = [{"program": 0}, {"program": 0, "fuse": 0}]
FP32_OPTIONS = [{}, {"trsm_wt_min": 1}]
_PLANS = {}


def get_plan(case):
    import cholesky_amd as ca
    if case not in _PLANS:
        _PLANS[case] = ca.Plan(*case_paths(case)[:3])
    return _PLANS[case]


def check_ranges(plan, options, f32):
    import cholesky_amd as ca
    dev = ca.Device(plan, 0)
    for name, value in options.items():
        dev.set_option(name, value)
    new, fill = (dev.new_arena_f32, dev.fill_f32) if f32 else (dev.new_arena, dev.fill)
    whole, levels = (dev.factor_f32, dev.factor_levels_f32) if f32 else (dev.factor, dev.factor_levels)
    L = plan.levels
    assert L >= 3

    def factored(*ranges):
        a = new()
        fill(a)
        for r in ranges:
            if r:
                levels(a, *r)
            else:
                whole(a)
        dev.sync()
        assert dev.info() == (0, 0), ranges
        return a

    one = factored((L - 1, 0))                                # (b)
    assert bool(one.isfinite().all())
    assert not one.equal(factored((L - 1, L - 1)))            # the comparison can tell a factor from a partly eliminated arena
    assert one.equal(factored(())), "whole-factor call"       # (a): fp32 always; fp64 with program: 0 it is the same path
    for k in range(1, L):                                     # (c)
        assert one.equal(factored((L - 1, k), (k - 1, 0))), f"cut at level {k} of {L}"
    assert one.equal(factored((L + 3, -2))), "range past both ends"


@pytest.mark.parametrize("options", FP64_OPTIONS, ids=["nofuse" if "fuse" in o else "default" for o in FP64_OPTIONS])
@pytest.mark.parametrize("case", PLANS)
def test_fp64_level_ranges_give_the_bits_of_the_whole_factor(case, options):
    check_ranges(get_plan(case), options, False)


@pytest.mark.parametrize("options", FP32_OPTIONS, ids=["wt_min_1" if o else "default" for o in FP32_OPTIONS])
@pytest.mark.parametrize("case", PLANS)
def test_fp32_level_ranges_give_the_bits_of_the_whole_factor(case, options):
    check_ranges(get_plan(case), options, True)
