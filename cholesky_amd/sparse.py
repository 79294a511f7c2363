"""Sparse solves on a factored A (include/cholamd.h at "sparse solves"): a right-hand side that is non-zero on a few dofs, a solution wanted on a few
dofs.  The sweeps touch the separators of those dofs and their ancestors only.  A ctypes mirror of cholamd_sparse_*, in the style of lowrank.py: torch
holds the device memory, every numeric step is a call into libcholamd.so."""
import ctypes as C

import numpy as np

from ._lib import check
from .device import Device, _stream_ptr
from .plan import Plan


class SparseSolve:
    """The pruned step lists of (in_dofs, out_dofs) -- original dof order, no duplicates inside either list -- on the device object `dev`, built and
    uploaded here: a warm solve_nrhs allocates nothing.  The handle refers to dev: close it first."""

    def __init__(self, dev, in_dofs, out_dofs):
        self.dev, self.L = dev, dev.L
        self.in_dofs, self.out_dofs = Plan._dofs(in_dofs, "in_dofs"), Plan._dofs(out_dofs, "out_dofs")
        h = C.c_void_p()
        check(self.L.cholamd_sparse_create(dev.h, self.in_dofs.ctypes.data, self.in_dofs.size, self.out_dofs.ctypes.data, self.out_dofs.size, C.byref(h)),
              "cholamd_sparse_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.cholamd_sparse_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def counts(self):
        """Plan.sparse_counts of the handle's lists (cholamd_sparse_counts)."""
        out = np.zeros(12, dtype=np.int64)
        check(self.L.cholamd_sparse_counts(self.h, out.ctypes.data), "cholamd_sparse_counts")
        return Plan._sparse_counts_dict(out)

    def solve_nrhs(self, arena, Bs, Xs, which=-1, stream=None):
        """Xs = rows out_dofs of A^-1 b (which = -1), M^-1 b (HALF_FORWARD) or M^-T b (HALF_BACKWARD), b = Bs on in_dofs and zero elsewhere.  Bs:
        len(in_dofs) x k, Xs: len(out_dofs) x k, column-major CUDA float64 (stride(0) == 1); Xs may be Bs where the two lists are equally long;
        asynchronous on `stream`."""
        ldb, k = Device._block(Bs, "Bs", self.in_dofs.size)
        ldx, kx = Device._block(Xs, "Xs", self.out_dofs.size)
        if kx != k:
            raise ValueError(f"Bs has {k} columns, Xs has {kx}")
        fn = self.L.cholamd_sparse_solve_nrhs_f32 if Device._is_f32(arena) else self.L.cholamd_sparse_solve_nrhs
        check(fn(self.h, Device.ptr(arena), Device.ptr(Bs), ldb, Device.ptr(Xs), ldx, k, int(which), _stream_ptr(stream)), "cholamd_sparse_solve_nrhs")

    def inverse_block(self, arena, stream=None):
        """A^-1[S, S] for S = in_dofs == out_dofs as an |S| x |S| CUDA tensor: the identity solved on the pruned lists."""
        import torch
        if not np.array_equal(self.in_dofs, self.out_dofs):
            raise ValueError("inverse_block needs in_dofs == out_dofs")
        m = self.in_dofs.size
        X = torch.eye(m, dtype=torch.float64, device=f"cuda:{self.dev.device_id}").T  # (column-major: stride(0) == 1)
        if stream is not None and hasattr(stream, "wait_stream"):
            stream.wait_stream(torch.cuda.current_stream(self.dev.device_id))  # (the identity was written on the current stream)
        self.solve_nrhs(arena, X, X, -1, stream)
        return X
