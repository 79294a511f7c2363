"""The device buffers a device object owns (cholesky_amd/csrc/chol_devbuf.h): every one of them goes with the object, the paths that rebuild the
schedule or the solve lists neither leak nor pile up, and the diagnostic program launch leaves nothing armed.

cholamd_debug_live_buffers() counts the library-owned device buffers of the whole process, so every check is a difference between two readings with
no other device object created or destroyed between them.  lapl_400x400 is the smallest fixture with five tree levels: a partition of 2 and a Schur
complement on k = 2 levels exist.  (The allocation-failure paths are covered on the host: tests/native/devbuf_host.cpp.)
"""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import case_paths  # noqa: E402
from test_gpu_factor import TOL_RESID  # noqa: E402

CASE = "lapl_400x400"


@pytest.fixture(scope="module")
def ca():
    import cholesky_amd
    return cholesky_amd


@pytest.fixture(scope="module")
def live(ca):
    from cholesky_amd._lib import load
    return load().cholamd_debug_live_buffers


@pytest.fixture(scope="module")
def plan(ca):
    m, o, c, _ = case_paths(CASE)
    return ca.Plan(m, o, c)


@pytest.fixture(scope="module")
def rhs(ca, plan):
    return ca.plan.read_vector(case_paths(CASE)[3], plan.n)


def destroy(dev):
    """cholamd_device_destroy now, not when the garbage collector gets to the object."""
    dev.L.cholamd_device_destroy(dev.h)
    dev.h = None


def factored(dev, arena=None):
    arena = dev.new_arena() if arena is None else arena
    dev.fill(arena)
    dev.factor(arena)
    dev.sync()
    assert dev.info() == (0, 0)
    return arena


def test_destroy_releases_every_lazily_built_group(ca, live, plan, rhs):
    import torch
    gc.collect()  # (device objects of earlier tests go now, not between the two readings)
    before = live()
    dev = ca.Device(plan, 0)
    assert live() > before
    n, F, B = plan.n, dev.HALF_FORWARD, dev.HALF_BACKWARD
    b = torch.from_numpy(rhs).cuda()
    x, r = torch.empty_like(b), torch.empty_like(b)
    B8 = torch.from_numpy(np.outer(np.arange(1.0, 9.0), rhs)).cuda().T  # n x 8, column-major: a chunk wide enough for the block kernels
    X8 = torch.empty(8, n, dtype=torch.float64, device="cuda").T

    arena = factored(dev)  # the program launch
    levels = dev.new_arena()
    dev.fill(levels)
    dev.factor_levels(levels, plan.levels - 1, 0)
    dev.sync()
    assert dev.info() == (0, 0)
    dev.solve(arena, b, x)
    dev.solve_nrhs(arena, B8, X8)
    dev.solve_half(arena, b, x, F)
    dev.solve_half(arena, x, x, B)
    assert np.isfinite(dev.logdet(arena))
    dev.factor_diag(arena)

    a32 = dev.new_arena_f32()
    dev.fill_f32(a32)
    dev.factor_f32(a32)
    assert dev.solve_refine(a32, b, x)[1] <= TOL_RESID
    assert dev.solve_refine_nrhs(a32, B8, X8)[1].max() <= TOL_RESID

    vals = np.ascontiguousarray(np.loadtxt(case_paths(CASE)[0], comments="%")[1:, 2])  # the matrix file's own values, in its order
    assert vals.size == plan.nz
    dev.set_values(vals)
    assert torch.equal(factored(dev, levels), arena)

    z = dev.selinv(arena)
    dev.selinv_entries(z)

    k = 2
    top = dev.new_arena()
    dev.fill(top)
    dev.schur_factor(top, k)
    S = dev.schur(top, k)
    w, g = dev.schur_condense(top, k, b)
    dev.schur_expand(top, k, w, torch.linalg.solve(S.cpu(), g.cpu()).cuda(), x)
    assert dev.residual(b, x, r) <= TOL_RESID

    dev.multiply(arena, b, x)
    assert dev.factor_residual(arena, b) <= TOL_RESID
    dev.fill(levels)
    assert len(dev.program_trace(levels)) > 0
    dev.sync()

    destroy(dev)
    assert live() == before


def test_rebuilds_neither_leak_nor_change_the_result(ca, live, plan, rhs, golden):
    import torch
    dev = ca.Device(plan, 0)
    b = torch.from_numpy(rhs).cuda()
    x = torch.empty_like(b)
    arena = factored(dev)
    L0 = arena.clone()
    dev.solve(arena, b, x)
    dev.sync()

    counts = []
    for _ in range(3):  # every set_option rebuilds the schedule
        pair = []
        for fuse in (0, 1):
            dev.set_option("fuse", fuse)
            factored(dev, arena)
            dev.solve(arena, b, x)
            dev.sync()
            pair.append(live())
        counts.append(pair)
    assert counts[1] == counts[0] and counts[2] == counts[0]

    dev.set_partition(1, 2)  # the schedule of rank 1 of 2, the solve lists dropped ...
    dev.set_partition(0, 1)  # ... and back: the solve rebuilds them
    dev.solve(arena, b, x)
    dev.sync()
    assert live() == counts[0][1]

    assert torch.equal(factored(dev, arena), L0)
    dev.solve(arena, b, x)
    dev.sync()
    g = golden(CASE)  # the residual as tests/test_gpu_factor.py takes it: A in original ordering
    A = g["pmat"] + np.tril(g["pmat"], -1).T
    Aorig = np.zeros_like(A)
    Aorig[np.ix_(plan.perm, plan.perm)] = A
    assert np.linalg.norm(Aorig @ x.cpu().numpy() - rhs) / np.linalg.norm(rhs) <= TOL_RESID
    destroy(dev)


def test_program_trace_leaves_nothing_armed(ca, live, plan):
    import torch
    dev = ca.Device(plan, 0)
    arena = factored(dev)
    L0 = arena.clone()
    count = live()
    dev.fill(arena)
    assert len(dev.program_trace(arena)) > 0
    assert live() == count  # the stamps went with the call
    assert torch.equal(factored(dev, arena), L0)  # a plain launch again: the diagnostic instance writes its stamps, this one has nowhere to
    destroy(dev)
