"""The three single-vector refinement entry points -- cholamd_solve_refine, cholamd_solve_refine_sharded and cholamd_solve_refine_multi -- run ONE loop
(refine_loop, chol_api_solve.cpp).  Pinned here through each door on an unpartitioned device object (the sharded door at world 1 returns before it reads
its communicator; the multi door takes a one-element device list), at n = 25 (one residual workgroup, every separator under one span) and n = 400.

The solves underneath add with fp64 atomics: the doors are compared by residual and against the golden x, never bit for bit.  The residual kernel has no
atomics, so the residual a door reports must EQUAL Device.residual of the iterate it returns."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import case_paths  # noqa: E402

CASES = ["lapl_25x25", "lapl_400x400"]
DOORS = ["single", "sharded", "multi"]
TOL, MAX_ITER = 1e-13, 20  # as in test_gpu_mixed.py
TOL_X = 1e-10              # ... and its gate on x


def refine(door, dev, a32, b, x, max_iter=MAX_ITER):
    from cholesky_amd.device import solve_refine_multi
    if door == "single":
        return dev.solve_refine(a32, b, x, max_iter=max_iter, tol=TOL)
    if door == "sharded":
        return dev.solve_refine_sharded(a32, b, x, None, max_iter=max_iter, tol=TOL)
    return solve_refine_multi([dev], [a32], [b], [x], max_iter=max_iter, tol=TOL)


def factored_f32(dev, a32=None):
    a32 = dev.new_arena_f32() if a32 is None else a32
    dev.fill_f32(a32)
    dev.factor_f32(a32)
    dev.sync()
    assert dev.info() == (0, 0)
    return a32


@pytest.fixture(scope="module", params=CASES)
def setup(request):
    """(case, plan, b on the device, the matrix file's values in its order)"""
    import torch
    import cholesky_amd as ca
    m, o, c, b = case_paths(request.param)
    plan = ca.Plan(m, o, c)
    vals = np.ascontiguousarray(np.loadtxt(m, comments="%")[1:, 2])
    assert vals.size == plan.nz
    return request.param, plan, torch.from_numpy(ca.plan.read_vector(b, plan.n)).cuda(), vals


def converged(door, dev, a32, d_b, gx):
    import torch
    d_x = torch.full_like(d_b, float("nan"))
    iters, rel = refine(door, dev, a32, d_b, d_x)
    assert 0 <= iters <= MAX_ITER and rel <= TOL, (door, iters, rel)
    assert np.abs(d_x.cpu().numpy() - gx).max() <= TOL_X * max(1.0, np.abs(gx).max()), door
    assert rel == dev.residual(d_b, d_x), door  # the reported number belongs to the returned iterate


@pytest.mark.parametrize("door", DOORS)
def test_three_doors_one_loop(setup, golden, door):
    import cholesky_amd as ca
    case, plan, d_b, _ = setup
    dev = ca.Device(plan, 0)
    converged(door, dev, factored_f32(dev), d_b, golden(case)["x"])


@pytest.mark.parametrize("max_iter", [0, -3])
@pytest.mark.parametrize("door", DOORS)
def test_no_correction_is_asked_for(setup, door, max_iter):
    import torch
    import cholesky_amd as ca
    _, plan, d_b, _ = setup
    dev = ca.Device(plan, 0)
    a32 = factored_f32(dev)
    d_x = torch.full_like(d_b, float("nan"))
    iters, rel = refine(door, dev, a32, d_b, d_x, max_iter=max_iter)
    assert iters == 0
    assert rel == dev.residual(d_b, d_x)


@pytest.fixture(scope="module")
def fresh_scaled(setup):
    """||b - 4 A x|| / ||b|| of ONE fp32-factor solve of the system with the fixture's values times 4, on a device object that has never refined"""
    import torch
    import cholesky_amd as ca
    _, plan, d_b, vals = setup
    dev = ca.Device(plan, 0)
    dev.set_values(4.0 * vals)
    a32 = factored_f32(dev)
    d_x = torch.empty_like(d_b)
    dev.solve_f32(a32, d_b, d_x)
    dev.sync()
    return dev.residual(d_b, d_x)


@pytest.mark.parametrize("door", DOORS)
def test_keep_inverses_does_not_leak_on_the_good_exit(setup, fresh_scaled, door):
    """After a refinement the next solve forms the diagonal inverses of ITS arena again: the same arena refactored from 4 A must solve 4 A x = b to the
    fp32 level a fresh object reaches (a kept inverse of A's factor is wrong by a factor of 2 in x)."""
    import torch
    import cholesky_amd as ca
    _, plan, d_b, vals = setup
    dev = ca.Device(plan, 0)
    a32 = factored_f32(dev)
    d_x = torch.empty_like(d_b)
    refine(door, dev, a32, d_b, d_x)
    dev.set_values(4.0 * vals)
    factored_f32(dev, a32)
    dev.solve_f32(a32, d_b, d_x)
    dev.sync()
    rel = dev.residual(d_b, d_x)
    print(f"{door}: {rel:.3e} after a refinement, {fresh_scaled:.3e} on a fresh object")
    assert rel <= 10.0 * fresh_scaled, (door, rel, fresh_scaled)


@pytest.mark.parametrize("door", DOORS)
def test_keep_inverses_does_not_leak_on_the_error_exit(setup, golden, door):
    import torch
    import cholesky_amd as ca
    case, plan, d_b, _ = setup
    dev = ca.Device(plan, 0)
    a32 = dev.new_arena_f32()
    a32.fill_(float("nan"))
    torch.cuda.synchronize()
    d_x = torch.empty_like(d_b)
    with pytest.raises(ca.CholamdError, match="produced NaN"):
        refine(door, dev, a32, d_b, d_x)
    dev.sync()
    factored_f32(dev, a32)
    converged("single", dev, a32, d_b, golden(case)["x"])
    if door != "single":  # ... and through the door that failed
        converged(door, dev, a32, d_b, golden(case)["x"])
