"""Low-rank corrections on a factored A (include/cholamd.h at "low-rank corrections"): solves, log det and variances of A + U U^T, A - U U^T and of A
under the linear constraints U^T x = e, with U a few dense columns.  A ctypes mirror of cholamd_lowrank_*, in the style of device.py: torch holds the
device memory, every numeric step is a call into libcholamd.so."""
import ctypes as C

import numpy as np

from ._lib import check
from .device import Device, _stream_ptr

UPDATE, DOWNDATE, CONSTRAINT = 1, -1, 0  # CHOLAMD_LOWRANK_UPDATE / _DOWNDATE / _CONSTRAINT
LOWRANK_MAX = 256                        # CHOLAMD_LOWRANK_MAX
_MODES = {"update": UPDATE, "downdate": DOWNDATE, "constraint": CONSTRAINT}


class LowRank:
    """W = A^-1 U L_C^-T for up to kmax columns of U on the device object `dev` (C = I + G, I - G or G = U^T A^-1 U by the mode).  After set(), solve() is
    one plain solve plus two passes over W.  W belongs to the arena's values at set() time: call set() again after a refactorisation."""

    def __init__(self, dev, kmax):
        self.dev, self.L, self.kmax = dev, dev.L, int(kmax)
        h = C.c_void_p()
        check(self.L.cholamd_lowrank_create(dev.h, int(kmax), C.byref(h)), "cholamd_lowrank_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.cholamd_lowrank_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def mode_of(mode):
        return _MODES[mode] if isinstance(mode, str) else int(mode)

    def _vec(self, t, what, count):
        import torch
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or not t.is_cuda or t.dim() != 1 or t.numel() != count or (count > 1 and t.stride(0) != 1):
            raise ValueError(f"{what} must be a contiguous 1-D CUDA float64 tensor of {count} elements")
        return Device.ptr(t)

    def set(self, arena, U, mode=UPDATE, stream=None):
        """U: n x k column-major CUDA float64 (stride(0) == 1).  Synchronises; raises CholamdError (state()[2] = the failing leading minor) and leaves the
        object unset when the capacitance matrix is not positive definite."""
        ldu, k = Device._block(U, "U", self.dev.plan.n)
        check(self.L.cholamd_lowrank_set(self.h, Device.ptr(arena), Device.ptr(U), ldu, k, self.mode_of(mode), _stream_ptr(stream)), "cholamd_lowrank_set")

    def state(self):
        """(k, mode, info of the last set); k == 0: unset."""
        out = (C.c_int * 3)()
        check(self.L.cholamd_lowrank_state(self.h, out), "cholamd_lowrank_state")
        return int(out[0]), int(out[1]), int(out[2])

    def solve(self, arena, b, x, e=None, stream=None):
        """x = A'^-1 b (constraint mode: the x of the KKT system with U^T x = e, e = None: zero); x may be b; asynchronous on `stream`."""
        n, k = self.dev.plan.n, self.state()[0]
        check(self.L.cholamd_lowrank_solve(self.h, Device.ptr(arena), self._vec(b, "b", n), None if e is None else self._vec(e, "e", k), self._vec(x, "x", n),
                                           _stream_ptr(stream)), "cholamd_lowrank_solve")

    def solve_nrhs(self, arena, B, X, E=None, stream=None):
        """The same for the columns of B (n x nrhs, column-major); E: k x nrhs column-major or None; X may be B."""
        ldb, ldx, nrhs = self.dev._blocks(B, X)
        pe, lde = None, self.state()[0]
        if E is not None:
            lde, ne = Device._block(E, "E", self.state()[0])
            if ne != nrhs:
                raise ValueError(f"B has {nrhs} columns, E has {ne}")
            pe = Device.ptr(E)
        check(self.L.cholamd_lowrank_solve_nrhs(self.h, Device.ptr(arena), Device.ptr(B), ldb, pe, lde, Device.ptr(X), ldx, nrhs, _stream_ptr(stream)),
              "cholamd_lowrank_solve_nrhs")

    def project(self, U, x, xout=None, e=None, stream=None):
        """x* = x - W L_C^-1 (U^T x - e) (constraint mode): the sample x put on the constraint set; xout may be x."""
        import torch
        n, k = self.dev.plan.n, self.state()[0]
        ldu, ku = Device._block(U, "U", n)
        if ku != k:
            raise ValueError(f"U has {ku} columns, the object was set with {k}")
        if xout is None:
            xout = torch.empty(n, dtype=torch.float64, device=x.device)
        check(self.L.cholamd_lowrank_project(self.h, Device.ptr(U), ldu, self._vec(x, "x", n), None if e is None else self._vec(e, "e", k),
                                             self._vec(xout, "xout", n), _stream_ptr(stream)), "cholamd_lowrank_project")
        return xout

    def diag(self, out=None, stream=None):
        """w_i = sum_j W_ij^2: diag(A'^-1) = diag(A^-1) - sigma w (sigma = -1 for a downdate, +1 otherwise)."""
        import torch
        n = self.dev.plan.n
        if out is None:
            out = torch.empty(n, dtype=torch.float64, device=f"cuda:{self.dev.device_id}")
        check(self.L.cholamd_lowrank_diag(self.h, self._vec(out, "out", n), _stream_ptr(stream)), "cholamd_lowrank_diag")
        return out

    def logdet_c(self):
        """log det C: log det(A +- U U^T) = Device.logdet(arena) + logdet_c()."""
        out = C.c_double(float("nan"))
        check(self.L.cholamd_lowrank_logdet(self.h, C.byref(out)), "cholamd_lowrank_logdet")
        return float(out.value)

    def factor(self):
        """L_C (k x k numpy, lower triangular)."""
        k = self.state()[0]
        out = np.zeros((max(k, 1), max(k, 1)), dtype=np.float64, order="F")
        check(self.L.cholamd_lowrank_factor(self.h, out.ctypes.data, max(k, 1)), "cholamd_lowrank_factor")
        return out

    def block(self):
        """The stored W as an n x k numpy array (a host copy)."""
        p, ld = C.c_void_p(), C.c_int64(0)
        check(self.L.cholamd_lowrank_block(self.h, C.byref(p), C.byref(ld)), "cholamd_lowrank_block")
        n, k = self.dev.plan.n, self.state()[0]
        self.dev.sync()
        return self.dev.download(p.value, ld.value * k).reshape(k, ld.value)[:, :n].T.copy()
