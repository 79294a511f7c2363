"""Host restatements of the low-rank kernels' partition (cholamd_lowrank_slabs, cholamd_lowrank_tprod_host, cholamd_lowrank_rprod_host): no device.

The slab partition of the transposed product is a function of n alone; the two products walk the kernels' own slabs, stage blocks, 4-row steps and 16-row
chunks.  Gates 1 and 2 of tests/lowrank_ref.py (inner-product bounds, valid for any summation order).  Every test prints its largest error / gate ratio with
pytest -s."""
import re

import numpy as np
import pytest

import lowrank_ref as lr
from conftest import ROOT

ERR_ARG = -4


@pytest.fixture(scope="module")
def L():
    import cholesky_amd
    return cholesky_amd.load()


def slab_size():
    with open(f"{ROOT}/cholesky_amd/csrc/chol_plan.h") as f:
        return int(re.search(r"#define CHOL_LR_SLAB (\d+)", f.read()).group(1))


S = slab_size()
SIZES = [1, 15, 16, 17, S - 1, S, S + 1, 2 * S - 1, 2 * S + 1, 3375]


def F(a):
    return np.asfortranarray(a, dtype=np.float64)


def padded(a, ld):
    """a (rows x cols) inside a Fortran block of ld rows whose padding rows are NaN."""
    out = np.full((ld, a.shape[1]), np.nan, order="F")
    out[:a.shape[0]] = a
    return out


@pytest.mark.parametrize("n", SIZES)
def test_slabs_cover_every_row_once_in_order(L, n):
    ns = L.cholamd_lowrank_slabs(n, None, 0)
    assert ns == -(-n // S)
    first = np.full(ns + 1, -1, dtype=np.int64)
    assert L.cholamd_lowrank_slabs(n, first.ctypes.data, ns) == ns
    assert first[ns] == -1                                     # cap is honoured
    ends = np.append(first[1:ns], n)
    rows = np.concatenate([np.arange(a, b) for a, b in zip(first[:ns], ends)])
    assert np.array_equal(rows, np.arange(n))
    assert np.all(ends - first[:ns] <= S) and np.all(ends[:-1] - first[:ns - 1] == S)
    short = np.full(2, -1, dtype=np.int64)                     # a short buffer: the count, the first `cap` entries
    assert L.cholamd_lowrank_slabs(n, short.ctypes.data, 1) == ns and short[0] == 0 and short[1] == -1


@pytest.mark.parametrize("n", SIZES)
def test_tprod_host_matches_numpy(L, n):
    rng = np.random.default_rng(n)
    worst = 0.0
    for k, m in [(1, 1), (17, 33), (33, 5)] + ([(256, 32)] if n in (17, S + 1) else []):
        P, Q = rng.standard_normal((n, k)), rng.standard_normal((n, m))
        Pp, Qp = padded(P, n + 3), padded(Q, n + 2)
        T = np.full((k + 1, m), np.nan, order="F")
        assert L.cholamd_lowrank_tprod_host(n, k, m, Pp.ctypes.data, n + 3, Qp.ctypes.data, n + 2, T.ctypes.data, k + 1) == 0
        assert np.all(np.isnan(T[k]))                          # the padding row is not written, the NaN rows behind n are not read
        worst = max(worst, lr.gate1_ratio(T[:k], P, Q))
        G = np.zeros((k, k), order="F")                        # the Gram form: P == Q
        assert L.cholamd_lowrank_tprod_host(n, k, k, Pp.ctypes.data, n + 3, Pp.ctypes.data, n + 3, G.ctypes.data, k) == 0
        assert np.array_equal(G, G.T)
        worst = max(worst, lr.gate1_ratio(G, P, P))
        Q2 = Qp.copy(order="F")                                # column independence: a NaN in a neighbouring column
        Q2[:, 0] = np.nan
        T2 = np.zeros((k, m), order="F")
        assert L.cholamd_lowrank_tprod_host(n, k, m, Pp.ctypes.data, n + 3, Q2.ctypes.data, n + 2, T2.ctypes.data, k) == 0
        assert np.array_equal(T2[:, 1:], T[:k, 1:]) and np.all(np.isnan(T2[:, 0]))
    print(f"tprod_host n = {n}: worst error / gate 1 = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("n", SIZES)
def test_rprod_host_matches_numpy(L, n):
    rng = np.random.default_rng(100 + n)
    worst = 0.0
    for k, m in [(1, 1), (17, 33), (33, 5)] + ([(256, 32)] if n in (17, S + 1) else []):
        V, T, X0 = rng.standard_normal((n, k)), rng.standard_normal((k, m)), rng.standard_normal((n, m))
        Vp, Tp = padded(V, n + 3), padded(T, k + 2)
        for alpha, beta in [(0.0, 1.0), (1.0, -1.0), (0.5, 2.0)]:
            X = padded(X0, n + 1)
            if alpha == 0.0:
                X[:] = np.nan                                  # alpha == 0: X is not read
            assert L.cholamd_lowrank_rprod_host(n, k, m, alpha, beta, Vp.ctypes.data, n + 3, Tp.ctypes.data, k + 2, X.ctypes.data, n + 1) == 0
            assert np.all(np.isnan(X[n]))
            worst = max(worst, lr.gate2_ratio(X[:n], alpha, X0, beta, V, T))
        R = F(rng.standard_normal((k, k)))                     # in place: V <- V R equals the out-of-place product bit for bit
        out, inp = np.zeros((n, k), order="F"), F(V)
        assert L.cholamd_lowrank_rprod_host(n, k, k, 0.0, 1.0, inp.ctypes.data, n, R.ctypes.data, k, out.ctypes.data, n) == 0
        assert L.cholamd_lowrank_rprod_host(n, k, k, 0.0, 1.0, inp.ctypes.data, n, R.ctypes.data, k, inp.ctypes.data, n) == 0
        assert np.array_equal(out, inp)
    print(f"rprod_host n = {n}: worst error / gate 2 = {worst:.3f}")
    assert worst <= 1.0


def test_argument_rules(L):
    a, t = F(np.arange(1.0, 7.0).reshape(3, 2)), F(np.full((2, 2), 9.0))
    A, T = a.ctypes.data, t.ctypes.data
    assert L.cholamd_lowrank_slabs(-1, None, 0) == ERR_ARG
    assert L.cholamd_lowrank_slabs(0, None, 0) == 0
    bad_t = [(3, 2, 2, A, 2, A, 3, T, 2), (3, 2, 2, A, 3, A, 2, T, 2), (3, 2, 2, A, 3, A, 3, T, 1), (3, 257, 2, A, 3, A, 3, T, 257), (-1, 2, 2, A, 3, A, 3, T, 2),
             (3, -1, 2, A, 3, A, 3, T, 2), (3, 2, -1, A, 3, A, 3, T, 2), (3, 2, 2, None, 3, A, 3, T, 2), (3, 2, 2, A, 3, None, 3, T, 2), (3, 2, 2, A, 3, A, 3, None, 2)]
    for args in bad_t:
        assert L.cholamd_lowrank_tprod_host(*args) == ERR_ARG, args
        assert L.cholamd_last_error()
    bad_r = [(3, 2, 2, 0.0, 1.0, A, 2, T, 2, A, 3), (3, 2, 2, 0.0, 1.0, A, 3, T, 1, A, 3), (3, 2, 2, 0.0, 1.0, A, 3, T, 2, A, 2), (3, 257, 2, 0.0, 1.0, A, 3, T, 257, A, 3),
             (3, 2, 2, 0.0, 1.0, None, 3, T, 2, A, 3), (3, 2, 2, 0.0, 1.0, A, 3, None, 2, A, 3), (3, 2, 2, 0.0, 1.0, A, 3, T, 2, None, 3)]
    for args in bad_r:
        assert L.cholamd_lowrank_rprod_host(*args) == ERR_ARG, args
    assert np.all(t == 9.0) and np.array_equal(a, np.arange(1.0, 7.0).reshape(3, 2))
    # k == 0 or m == 0: 0, nothing touched; n == 0: T = 0
    assert L.cholamd_lowrank_tprod_host(3, 0, 2, A, 3, A, 3, T, 1) == 0 and L.cholamd_lowrank_rprod_host(3, 2, 0, 0.0, 1.0, A, 3, T, 2, A, 3) == 0
    assert np.all(t == 9.0)
    assert L.cholamd_lowrank_tprod_host(0, 2, 2, A, 1, A, 1, T, 2) == 0 and np.all(t == 0.0)
