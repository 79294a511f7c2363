"""Device-side driver objects: the level schedule of mmat.rg:1227-1355 on one MI355X.

torch is used for what it is good at here -- device buffers, streams, torch.distributed (RCCL) --
and every numeric step is a call into libcholamd.so with raw pointers."""
import ctypes as C

import numpy as np

from ._lib import check, load

_check = check  # Device.set_values has a parameter of that name

HALF_FORWARD, HALF_BACKWARD = 0, 1  # CHOLAMD_HALF_FORWARD (x = M^-1 b), CHOLAMD_HALF_BACKWARD (x = M^-T b); M = P^T L P


def _stream_ptr(stream):
    if stream is None:
        return None
    if hasattr(stream, "cuda_stream"):
        return C.c_void_p(stream.cuda_stream)
    return C.c_void_p(int(stream))


class RankArena:
    """A device arena owned by the library (Device.alloc_arena): data_ptr() like a tensor, numpy() = a host copy of the whole address range."""

    def __init__(self, dev, ptr, elem_bytes, backed_bytes):
        self.dev, self._ptr, self.elem_bytes, self.backed_bytes = dev, ptr, elem_bytes, backed_bytes
        self.nbytes = dev.plan.arena_doubles * elem_bytes

    def data_ptr(self):
        return self._ptr

    def numpy(self):
        n = self.dev.plan.arena_doubles
        out = np.empty(n, dtype=np.float64 if self.elem_bytes == 8 else np.float32)
        words = out.nbytes // 8  # cholamd_device_download counts doubles (the fp32 arena of an even number of floats, or its last float stays behind)
        check(self.dev.L.cholamd_device_download(self.dev.h, out.ctypes.data, C.c_void_p(self._ptr), words, None), "download")
        return out

    def free(self):
        if self._ptr:
            check(self.dev.L.cholamd_device_free_arena(self.dev.h, C.c_void_p(self._ptr)), "cholamd_device_free_arena")
            self._ptr = 0


class Device:
    KINDS = ("potrf", "trsm", "update", "other")

    def __init__(self, plan, device_id=0):
        self.L = load()
        self.plan = plan
        self.device_id = device_id
        h = C.c_void_p()
        check(self.L.cholamd_device_create(plan.h, device_id, C.byref(h)), "cholamd_device_create")
        self.h = h
        self._owned = []
        self._values_buf = None  # set_values: the device copy of a host value array

    def __del__(self):
        try:
            if getattr(self, "h", None):
                for p in self._owned:
                    self.L.cholamd_device_free(self.h, p)
                self.L.cholamd_device_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # -- memory ---------------------------------------------------------------------------------
    def alloc(self, doubles):
        """Library-owned device buffer (hipMalloc); returns the raw pointer as int."""
        p = C.c_void_p()
        check(self.L.cholamd_device_alloc(self.h, int(doubles), C.byref(p)), "cholamd_device_alloc")
        self._owned.append(p)
        return p.value

    def new_arena(self):
        """A torch fp64 CUDA tensor of the arena size (caller-owned buffer, like Legion's regions)."""
        import torch
        return torch.empty(self.plan.arena_doubles, dtype=torch.float64, device=f"cuda:{self.device_id}")

    def alloc_arena(self, elem_bytes=8):
        """This rank's arena by cholamd_device_alloc_arena: complete address range, memory of its own only under the rank's panels and the shared
        top (the other ranks' panels alias one scratch chunk); rank 0 / single GPU: a plain allocation.  Returns a RankArena."""
        p, backed = C.c_void_p(), C.c_int64(0)
        check(self.L.cholamd_device_alloc_arena(self.h, int(elem_bytes), C.byref(p), C.byref(backed)), "cholamd_device_alloc_arena")
        return RankArena(self, p.value, int(elem_bytes), backed.value)

    @staticmethod
    def ptr(t):
        return C.c_void_p(t if isinstance(t, int) else t.data_ptr())

    def upload(self, dptr, host, stream=None):
        host = np.ascontiguousarray(host, dtype=np.float64)
        check(self.L.cholamd_device_upload(self.h, self.ptr(dptr), host.ctypes.data, host.size, _stream_ptr(stream)), "upload")

    def download(self, dptr, doubles, stream=None):
        out = np.empty(int(doubles), dtype=np.float64)
        check(self.L.cholamd_device_download(self.h, out.ctypes.data, self.ptr(dptr), out.size, _stream_ptr(stream)), "download")
        return out

    def sync(self, stream=None):
        check(self.L.cholamd_device_sync(self.h, _stream_ptr(stream)), "sync")

    # -- the path -------------------------------------------------------------------------------
    def fill(self, arena, stream=None):
        """A scatter on the device: fill_block for every block (mmat.rg:1216-1224)."""
        check(self.L.cholamd_device_fill(self.h, self.ptr(arena), _stream_ptr(stream)), "cholamd_device_fill")

    VALUES_NOCHECK = 1  # CHOLAMD_VALUES_NOCHECK
    HALF_FORWARD, HALF_BACKWARD = 0, 1  # CHOLAMD_HALF_FORWARD / CHOLAMD_HALF_BACKWARD

    def set_values(self, values, check=True, stream=None):
        """New values of A on the plan's pattern (cholamd_device_set_values): `values` is the value array of plan.nz doubles in the order of
        plan.entries() -- a contiguous 1-D float64 tensor on this device is read where it is, a 1-D float64 numpy array is uploaded through a
        buffer this object keeps.  Anything else raises ValueError.  Fill and factor afterwards; residuals and refinements measure against the
        new A.  check=True synchronises once and refuses (CholamdError, previous values kept) an array that gives an out-of-pattern entry a
        non-zero value; check=False is asynchronous on `stream` and ignores such values (values_status() reports them)."""
        import torch
        nz = self.plan.nz
        if isinstance(values, np.ndarray):
            if values.dtype != np.float64 or values.ndim != 1 or values.size != nz or not values.flags.c_contiguous:
                raise ValueError(f"values must be a contiguous 1-D float64 array of plan.nz = {nz} elements; got {values.dtype} {values.shape}")
            if self._values_buf is None:
                self._values_buf = torch.empty(max(nz, 1), dtype=torch.float64, device=f"cuda:{self.device_id}")
            self.upload(self._values_buf, values, stream)
            ptr = self._values_buf.data_ptr()
        elif isinstance(values, torch.Tensor):
            if values.dtype != torch.float64 or values.dim() != 1 or values.numel() != nz or not values.is_contiguous():
                raise ValueError(f"values must be a contiguous 1-D float64 tensor of plan.nz = {nz} elements; got {values.dtype} {tuple(values.shape)} strides {values.stride()}")
            if not values.is_cuda or values.device.index != self.device_id:
                raise ValueError(f"values must live on cuda:{self.device_id}; got {values.device}")
            ptr = values.data_ptr()
        else:
            raise ValueError("values must be a float64 numpy array or CUDA tensor")
        _check(self.L.cholamd_device_set_values(self.h, C.c_void_p(ptr), nz, 0 if check else self.VALUES_NOCHECK, _stream_ptr(stream)),
               "cholamd_device_set_values")

    def values_status(self, stream=None):
        """(in-pattern values that are non-zero and not a normal float in magnitude, the first one's value-array index or -1, out-of-pattern
        entries whose value is not zero, the first one's index or -1) of the last set_values call (cholamd_device_values_status)."""
        out = np.zeros(4, dtype=np.int64)
        _check(self.L.cholamd_device_values_status(self.h, _stream_ptr(stream), out.ctypes.data), "cholamd_device_values_status")
        return tuple(int(v) for v in out)

    def factor(self, arena, stream=None):
        """The level loop (mmat.rg:1227-1355), asynchronous on `stream`."""
        check(self.L.cholamd_factor(self.h, self.ptr(arena), _stream_ptr(stream)), "cholamd_factor")

    def factor_levels(self, arena, level_hi, level_lo, stream=None):
        check(self.L.cholamd_factor_levels(self.h, self.ptr(arena), level_hi, level_lo, _stream_ptr(stream)), "cholamd_factor_levels")

    def set_partition(self, rank, world):
        check(self.L.cholamd_device_set_partition(self.h, rank, world), "cholamd_device_set_partition")

    def dist_top_active(self):
        """True when the partitioned schedule holds broadcast phases (top levels distributed by column blocks)."""
        return self.L.cholamd_device_bcast_phases(self.h) > 0

    def set_option(self, name, value):
        """Schedule / kernel-selection switch of this device object (cholamd_device_set_option).  Among them "solve_deterministic" (the same bits from
        every single-vector solve) and, on top of it, "solve_deterministic_block": the _nrhs solves then take the deterministic block path -- one
        pass over the factor per 32 columns, the same bits every time, every column's bits independent of the other columns (include/cholamd.h at
        "deterministic solve"), and "schur_deterministic": schur_condense / schur_expand and their _nrhs forms walk deterministic step lists cut at
        the kept levels -- the same bits every time, columns independent, S never read (include/cholamd.h at cholamd_schur_condense_nrhs)."""
        check(self.L.cholamd_device_set_option(self.h, name.encode(), int(value)), "cholamd_device_set_option")

    def program_trace(self, arena, stream=None):
        """Diagnostic: one program launch with per-job stamps -> int64 array [jobs, 5] = kind, drawn, waits over, ended (10 ns ticks), workgroup."""
        n = C.c_int(0)
        check(self.L.cholamd_device_program_trace(self.h, self.ptr(arena), _stream_ptr(stream), 0, None, C.byref(n)), "cholamd_device_program_trace")
        out = np.zeros((n.value, 5), dtype=np.int64)
        check(self.L.cholamd_device_program_trace(self.h, self.ptr(arena), _stream_ptr(stream), out.size, out.ctypes.data, C.byref(n)), "cholamd_device_program_trace")
        return out

    def tail_offset(self):
        """First double of the shared top of the tree in the arena under the current partition."""
        return int(self.L.cholamd_device_tail_offset(self.h))

    def exchange_tail(self, arena, comm, stream=None):
        """The extend-add exchange alone: in-place RCCL all-reduce (sum) of the arena tail (cholamd_exchange_tail)."""
        check(self.L.cholamd_exchange_tail(self.h, self.ptr(arena), comm.h, _stream_ptr(stream)), "cholamd_exchange_tail")

    def factor_sharded(self, arena, comm, stream=None):
        """This rank's part of a sharded factorisation (cholamd_factor_sharded): local levels, RCCL exchange, top levels."""
        check(self.L.cholamd_factor_sharded(self.h, self.ptr(arena), comm.h if comm is not None else None, _stream_ptr(stream)), "cholamd_factor_sharded")

    def factor_sharded_f32(self, arena32, comm, stream=None):
        """The same with the fp32 factor (cholamd_factor_sharded_f32): mixed precision x multi-GPU."""
        check(self.L.cholamd_factor_sharded_f32(self.h, self.ptr(arena32), comm.h if comm is not None else None, _stream_ptr(stream)), "cholamd_factor_sharded_f32")

    def gather_to_root(self, arena, comm, stream=None):
        """The subtree panels this rank owns -> rank 0's arena (cholamd_gather_to_root); fp64 or fp32 arena by the tensor's dtype."""
        check(self.L.cholamd_gather_to_root(self.h, self.ptr(arena), int(arena.element_size()), comm.h, _stream_ptr(stream)), "cholamd_gather_to_root")

    def exchange_volume(self):
        """(received, sent, tail, pieces) in elements of the extend-add exchange of this rank's partition (cholamd_exchange_volume)."""
        out = np.zeros(4, dtype=np.int64)
        check(self.L.cholamd_exchange_volume(self.h, out.ctypes.data), "cholamd_exchange_volume")
        return tuple(int(v) for v in out)

    def info(self):
        sep = C.c_int(0)
        rc = self.L.cholamd_factor_info(self.h, C.byref(sep))
        if rc < 0:
            check(rc, "cholamd_factor_info")
        return rc, sep.value

    def solve(self, arena, b, x, stream=None):
        check(self.L.cholamd_solve(self.h, self.ptr(arena), self.ptr(b), self.ptr(x), _stream_ptr(stream)), "cholamd_solve")

    # -- mixed precision: fp32 factor + fp64 iterative refinement (BASELINE config 5) -----------------
    def new_arena_f32(self):
        import torch
        return torch.empty(self.plan.arena_doubles, dtype=torch.float32, device=f"cuda:{self.device_id}")

    def fill_f32(self, arena32, stream=None):
        check(self.L.cholamd_device_fill_f32(self.h, self.ptr(arena32), _stream_ptr(stream)), "cholamd_device_fill_f32")

    def factor_f32(self, arena32, stream=None):
        check(self.L.cholamd_factor_f32(self.h, self.ptr(arena32), _stream_ptr(stream)), "cholamd_factor_f32")

    def factor_levels_f32(self, arena32, level_hi, level_lo, stream=None):
        check(self.L.cholamd_factor_levels_f32(self.h, self.ptr(arena32), level_hi, level_lo, _stream_ptr(stream)), "cholamd_factor_levels_f32")

    def solve_f32(self, arena32, b, x, stream=None):
        check(self.L.cholamd_solve_f32(self.h, self.ptr(arena32), self.ptr(b), self.ptr(x), _stream_ptr(stream)), "cholamd_solve_f32")

    def solve_refine(self, arena32, b, x, max_iter=20, tol=1e-12, stream=None):
        """x = A^-1 b by iterative refinement on the fp32 factor; returns (corrections applied, ||b - A x|| / ||b||)."""
        it, rel = C.c_int(0), C.c_double(0.0)
        check(self.L.cholamd_solve_refine(self.h, self.ptr(arena32), self.ptr(b), self.ptr(x), int(max_iter), float(tol),
                                          C.byref(it), C.byref(rel), _stream_ptr(stream)), "cholamd_solve_refine")
        return it.value, rel.value

    def solve_sharded(self, arena, b, x, comm, stream=None):
        """This rank's part of the distributed solve (cholamd_solve_sharded / _f32 by the arena's element type): only vectors travel."""
        import torch
        f32 = arena.elem_bytes == 4 if isinstance(arena, RankArena) else arena.dtype == torch.float32
        fn = self.L.cholamd_solve_sharded_f32 if f32 else self.L.cholamd_solve_sharded
        check(fn(self.h, self.ptr(arena), self.ptr(b), self.ptr(x), comm.h if comm is not None else None, _stream_ptr(stream)), "cholamd_solve_sharded")

    def solve_refine_sharded(self, arena32, b, x, comm, max_iter=20, tol=1e-12, stream=None):
        """cholamd_solve_refine_sharded: the fp64 refinement with the fp32 factor left on the ranks; returns (corrections, relres)."""
        it, rel = C.c_int(0), C.c_double(0.0)
        check(self.L.cholamd_solve_refine_sharded(self.h, self.ptr(arena32), self.ptr(b), self.ptr(x), max_iter, tol, C.byref(it), C.byref(rel),
                                                  comm.h if comm is not None else None, _stream_ptr(stream)), "cholamd_solve_refine_sharded")
        return int(it.value), float(rel.value)

    @staticmethod
    def _block(t, what, n):
        """(ld, nrhs) of a 2-D column-major float64 CUDA tensor of n rows (stride(0) == 1, ld = stride(1)); ValueError otherwise."""
        import torch
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or not t.is_cuda or t.dtype != torch.float64:
            raise ValueError(f"{what} must be a 2-D CUDA float64 tensor, e.g. torch.empty(k, n).T")
        if t.shape[0] != n:
            raise ValueError(f"{what} has {t.shape[0]} rows, the system has n = {n}")
        if t.shape[1] > 0 and t.stride(0) != 1:
            raise ValueError(f"{what} must be column-major (stride(0) == 1), e.g. torch.empty(k, n).T; got strides {t.stride()}")
        if t.shape[1] > 1 and t.stride(1) < n:  # overlapping columns (expand, as_strided): the library would read / write k * ld doubles
            raise ValueError(f"{what} has column stride {t.stride(1)} < n = {n}: its columns overlap")
        return (int(t.stride(1)) if t.shape[1] > 1 else n), int(t.shape[1])

    def _blocks(self, B, X):
        ldb, k = self._block(B, "B", self.plan.n)
        ldx, kx = self._block(X, "X", self.plan.n)
        if kx != k:
            raise ValueError(f"B has {k} columns, X has {kx}")
        return ldb, ldx, k

    def solve_nrhs(self, arena, B, X, stream=None):
        """X = A^-1 B for the k columns of B (n x k, column-major: stride(0) == 1) in one pass over the factor per 32 columns
        (cholamd_solve_nrhs / _f32 by the arena's element type); asynchronous on `stream`.  Under option solve_deterministic: column by column, or, with
        solve_deterministic_block set too, the deterministic block path (bit-reproducible, columns independent of each other)."""
        import torch
        ldb, ldx, k = self._blocks(B, X)
        f32 = arena.elem_bytes == 4 if isinstance(arena, RankArena) else arena.dtype == torch.float32
        fn = self.L.cholamd_solve_nrhs_f32 if f32 else self.L.cholamd_solve_nrhs
        check(fn(self.h, self.ptr(arena), self.ptr(B), ldb, self.ptr(X), ldx, k, _stream_ptr(stream)), "cholamd_solve_nrhs")

    # -- one triangular half of the solve, the factor's diagonal, log det A (M = P^T L P, M M^T = A in original dof order) ------------
    @staticmethod
    def _is_f32(arena):
        import torch
        return arena.elem_bytes == 4 if isinstance(arena, RankArena) else arena.dtype == torch.float32

    def solve_half(self, arena, b, x, which, stream=None):
        """x = M^-1 b (which = HALF_FORWARD) or x = M^-T b (HALF_BACKWARD): cholamd_solve_half / _f32 by the arena's element type; x may be b."""
        fn = self.L.cholamd_solve_half_f32 if self._is_f32(arena) else self.L.cholamd_solve_half
        check(fn(self.h, self.ptr(arena), self.ptr(b), self.ptr(x), int(which), _stream_ptr(stream)), "cholamd_solve_half")

    def solve_half_nrhs(self, arena, B, X, which, stream=None):
        """The same for the k columns of B (n x k, column-major, as solve_nrhs takes them): cholamd_solve_half_nrhs / _f32.  With the options
        solve_deterministic and solve_deterministic_block BACKWARD of FORWARD of B equals solve_nrhs(B) bit for bit."""
        ldb, ldx, k = self._blocks(B, X)
        fn = self.L.cholamd_solve_half_nrhs_f32 if self._is_f32(arena) else self.L.cholamd_solve_half_nrhs
        check(fn(self.h, self.ptr(arena), self.ptr(B), ldb, self.ptr(X), ldx, k, int(which), _stream_ptr(stream)), "cholamd_solve_half_nrhs")

    def logdet(self, arena, stream=None):
        """log det A = 2 sum log L_ii from the factor in `arena` (cholamd_factor_logdet / _f32); synchronises `stream`; deterministic."""
        out = C.c_double(float("nan"))
        fn = self.L.cholamd_factor_logdet_f32 if self._is_f32(arena) else self.L.cholamd_factor_logdet
        check(fn(self.h, self.ptr(arena), C.byref(out), _stream_ptr(stream)), "cholamd_factor_logdet")
        return float(out.value)

    def factor_diag(self, arena, out=None, stream=None):
        """diag(M): out[dof] = L(p, p), p the permuted position of dof (cholamd_factor_diag / _f32), a float64 CUDA tensor of n elements;
        asynchronous on `stream`."""
        import torch
        n = self.plan.n
        if out is None:
            out = torch.empty(n, dtype=torch.float64, device=f"cuda:{self.device_id}")
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or not out.is_cuda or out.dim() != 1 or out.numel() != n or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous 1-D CUDA float64 tensor of n = {n} elements")
        fn = self.L.cholamd_factor_diag_f32 if self._is_f32(arena) else self.L.cholamd_factor_diag
        check(fn(self.h, self.ptr(arena), self.ptr(out), _stream_ptr(stream)), "cholamd_factor_diag")
        return out

    # -- the factor applied forwards: y = M z, M^T z, M M^T z (deterministic: one owner per element, no atomics) ---------------------------
    def multiply_half(self, arena, z, y, which, stream=None):
        """y = M z (which = HALF_FORWARD) or y = M^T z (HALF_BACKWARD): cholamd_multiply_half / _f32 by the arena's element type, the inverse of
        solve_half(which); y may be z.  Asynchronous on `stream`."""
        n = self.plan.n
        self._f64_vec(z, "z", n)
        self._f64_vec(y, "y", n)
        fn = self.L.cholamd_multiply_half_f32 if self._is_f32(arena) else self.L.cholamd_multiply_half
        check(fn(self.h, self.ptr(arena), self.ptr(z), self.ptr(y), int(which), _stream_ptr(stream)), "cholamd_multiply_half")

    def multiply(self, arena, z, y, stream=None):
        """y = M M^T z, which is A z up to the factorisation's backward error (cholamd_multiply / _f32); y may be z.  Asynchronous on `stream`."""
        n = self.plan.n
        self._f64_vec(z, "z", n)
        self._f64_vec(y, "y", n)
        fn = self.L.cholamd_multiply_f32 if self._is_f32(arena) else self.L.cholamd_multiply
        check(fn(self.h, self.ptr(arena), self.ptr(z), self.ptr(y), _stream_ptr(stream)), "cholamd_multiply")

    def multiply_half_nrhs(self, arena, Z, Y, which, stream=None):
        """Y = M Z (which = HALF_FORWARD) or Y = M^T Z (HALF_BACKWARD) for the k columns of Z (n x k, column-major, as solve_half_nrhs takes them) in one
        pass over the factor per 32 columns: cholamd_multiply_half_nrhs / _f32 by the arena's element type; Y may be Z.  Asynchronous on `stream`."""
        ldz, ldy, k = self._blocks(Z, Y)
        fn = self.L.cholamd_multiply_half_nrhs_f32 if self._is_f32(arena) else self.L.cholamd_multiply_half_nrhs
        check(fn(self.h, self.ptr(arena), self.ptr(Z), ldz, self.ptr(Y), ldy, k, int(which), _stream_ptr(stream)), "cholamd_multiply_half_nrhs")

    def multiply_nrhs(self, arena, Z, Y, stream=None):
        """Y = M M^T Z for the k columns of Z (cholamd_multiply_nrhs / _f32); Y may be Z.  Asynchronous on `stream`."""
        ldz, ldy, k = self._blocks(Z, Y)
        fn = self.L.cholamd_multiply_nrhs_f32 if self._is_f32(arena) else self.L.cholamd_multiply_nrhs
        check(fn(self.h, self.ptr(arena), self.ptr(Z), ldz, self.ptr(Y), ldy, k, _stream_ptr(stream)), "cholamd_multiply_nrhs")

    def factor_residual(self, arena, z, stream=None):
        """||A z - M M^T z|| / ||A z|| for the probe z, A with the device object's CURRENT values (cholamd_factor_residual / _f32): does `arena` factor
        them, and how well.  Synchronises `stream`; deterministic."""
        self._f64_vec(z, "z", self.plan.n)
        out = C.c_double(float("nan"))
        fn = self.L.cholamd_factor_residual_f32 if self._is_f32(arena) else self.L.cholamd_factor_residual
        check(fn(self.h, self.ptr(arena), self.ptr(z), C.byref(out), _stream_ptr(stream)), "cholamd_factor_residual")
        return float(out.value)

    # -- selected inversion: the entries of A^-1 on the pattern of the factor ---------------------------------------------------------
    def _f64_vec(self, t, what, count):
        import torch
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or not t.is_cuda or t.dim() != 1 or t.numel() != count or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous 1-D CUDA float64 tensor of {count} elements")
        return t

    def selinv(self, arena, zarena=None, stream=None):
        """Z = (P A P^T)^-1 on the pattern of L from the fp64 factor in `arena` (cholamd_selinv), into `zarena` (a second arena: the arena's own
        layout, plan.arena_to_dense reads it; allocated when None) -- returned.  Asynchronous on `stream`; deterministic."""
        if zarena is None:
            zarena = self.new_arena()
        check(self.L.cholamd_selinv(self.h, self.ptr(arena), self.ptr(zarena), _stream_ptr(stream)), "cholamd_selinv")
        return zarena

    def selinv_diag(self, zarena, out=None, stream=None):
        """diag(A^-1) in original dof order from the Z arena of selinv (cholamd_selinv_diag): a float64 CUDA tensor of n elements."""
        import torch
        if out is None:
            out = torch.empty(self.plan.n, dtype=torch.float64, device=f"cuda:{self.device_id}")
        self._f64_vec(out, "out", self.plan.n)
        check(self.L.cholamd_selinv_diag(self.h, self.ptr(zarena), self.ptr(out), _stream_ptr(stream)), "cholamd_selinv_diag")
        return out

    def selinv_entries(self, zarena, out=None, stream=None):
        """(A^-1)(row_k, col_k) for every entry k of plan.entries() (the value-array order of set_values) from the Z arena of selinv
        (cholamd_selinv_entries); NaN for the entries outside the pattern or dropped by the ordering.  A float64 CUDA tensor of plan.nz elements."""
        import torch
        if out is None:
            out = torch.empty(self.plan.nz, dtype=torch.float64, device=f"cuda:{self.device_id}")
        self._f64_vec(out, "out", self.plan.nz)
        check(self.L.cholamd_selinv_entries(self.h, self.ptr(zarena), self.ptr(out), self.plan.nz, _stream_ptr(stream)), "cholamd_selinv_entries")
        return out

    # -- gradients with respect to the value array: the contraction of an adjoint onto the entries of A(v) ---------------------------------
    def values_grad_pairs(self, P, Q, alpha=1.0, beta=0.0, out=None, stream=None):
        """out[k] = alpha * sum_c (P[i, c] Q[j, c] + P[j, c] Q[i, c]) + beta * out[k] for every entry k at (i, j) of plan.entries() (one product on the
        diagonal, 0 outside the pattern): cholamd_values_grad_pairs.  P, Q: n x nrhs column-major (as solve_nrhs takes them; P may be Q); out: plan.nz
        doubles, allocated when None (then beta must be 0), returned.  With X = A^-1 B and Lam = A^-1 dloss/dX: dloss/dvalues = values_grad_pairs(Lam,
        X, alpha=-1).  Asynchronous on `stream`; deterministic.  Refuses plans with dropped or duplicate entries (CholamdError)."""
        import torch
        (ldp, k), (ldq, kq) = self._block(P, "P", self.plan.n), self._block(Q, "Q", self.plan.n)
        if kq != k:
            raise ValueError(f"P has {k} columns, Q has {kq}")
        if out is None:
            if beta != 0.0:
                raise ValueError("beta != 0 needs the array to accumulate into (out)")
            out = (torch.empty if k else torch.zeros)(self.plan.nz, dtype=torch.float64, device=f"cuda:{self.device_id}")  # (no columns: the call touches nothing)
        self._f64_vec(out, "out", self.plan.nz)
        check(self.L.cholamd_values_grad_pairs(self.h, self.ptr(P), ldp, self.ptr(Q), ldq, k, float(alpha), float(beta), self.ptr(out), self.plan.nz,
                                               _stream_ptr(stream)), "cholamd_values_grad_pairs")
        return out

    def values_grad_logdet(self, zarena, alpha=1.0, beta=0.0, out=None, stream=None):
        """out[k] = alpha * m_k (A^-1)(i, j) + beta * out[k] = alpha * d(log det A)/dvalues[k] + beta * out[k] from the Z arena of selinv (m_k = 2 off
        the diagonal, 1 on it; 0 outside the pattern): cholamd_values_grad_logdet.  out as for values_grad_pairs.  Asynchronous; deterministic."""
        import torch
        if out is None:
            if beta != 0.0:
                raise ValueError("beta != 0 needs the array to accumulate into (out)")
            out = torch.empty(self.plan.nz, dtype=torch.float64, device=f"cuda:{self.device_id}")
        self._f64_vec(out, "out", self.plan.nz)
        check(self.L.cholamd_values_grad_logdet(self.h, self.ptr(zarena), float(alpha), float(beta), self.ptr(out), self.plan.nz, _stream_ptr(stream)),
              "cholamd_values_grad_logdet")
        return out

    # -- Schur complement on the top k levels of the tree: S = A_TT - A_TI A_II^-1 A_IT, condense, expand ---------------------------
    def schur_factor(self, arena, k, stream=None):
        """Eliminate the tree levels levels - 1 .. k of a filled fp64 arena by the per-level launches (cholamd_schur_factor): the blocks of the k kept
        levels then hold S.  factor_levels(arena, k - 1, 0) afterwards completes the factor.  Asynchronous on `stream`."""
        check(self.L.cholamd_schur_factor(self.h, self.ptr(arena), int(k), _stream_ptr(stream)), "cholamd_schur_factor")

    def schur(self, arena, k, out=None, stream=None):
        """S as an m x m column-major float64 CUDA tensor (stride(0) == 1), both triangles, in the Schur order of plan.schur_dofs(k) (cholamd_schur).
        `out`: a 2-D column-major tensor of m columns and at least m rows -- the rows beyond m are never touched; allocated when None.  fp64 arena
        only.  Asynchronous on `stream`; deterministic.  Returns the m x m view."""
        import torch
        if self._is_f32(arena):
            raise ValueError("schur needs the fp64 arena (there is no fp32 form of cholamd_schur)")
        m = self.plan.schur_size(k)
        if out is None:
            out = torch.empty((m, m), dtype=torch.float64, device=f"cuda:{self.device_id}").T
        if not isinstance(out, torch.Tensor) or out.dim() != 2 or not out.is_cuda or out.dtype != torch.float64:
            raise ValueError("out must be a 2-D CUDA float64 tensor, e.g. torch.empty(m, lds).T")
        if out.shape[1] != m or out.shape[0] < m:
            raise ValueError(f"out has shape {tuple(out.shape)}, S is {m} x {m}")
        if m > 0 and out.stride(0) != 1:
            raise ValueError(f"out must be column-major (stride(0) == 1), e.g. torch.empty(m, lds).T; got strides {out.stride()}")
        if m > 1 and out.stride(1) < out.shape[0]:
            raise ValueError(f"out has column stride {out.stride(1)} < its {out.shape[0]} rows: its columns overlap")
        lds = int(out.stride(1)) if m > 1 else max(int(out.shape[0]), 1)
        check(self.L.cholamd_schur(self.h, self.ptr(arena), int(k), self.ptr(out), lds, _stream_ptr(stream)), "cholamd_schur")
        return out[:m, :]

    def schur_condense(self, arena, k, b, w=None, g=None, stream=None):
        """g = b_T - A_TI A_II^-1 b_I (m doubles, Schur order) and the state w of schur_expand (n doubles) from b (n doubles, original dof order):
        cholamd_schur_condense / _f32 by the arena's element type.  w and g are allocated when None; returns (w, g).  Asynchronous on `stream`."""
        import torch
        n, m = self.plan.n, self.plan.schur_size(k)
        self._f64_vec(b, "b", n)
        w = torch.empty(n, dtype=torch.float64, device=f"cuda:{self.device_id}") if w is None else self._f64_vec(w, "w", n)
        g = torch.empty(m, dtype=torch.float64, device=f"cuda:{self.device_id}") if g is None else self._f64_vec(g, "g", m)
        fn = self.L.cholamd_schur_condense_f32 if self._is_f32(arena) else self.L.cholamd_schur_condense
        check(fn(self.h, self.ptr(arena), int(k), self.ptr(b), self.ptr(w), self.ptr(g), _stream_ptr(stream)), "cholamd_schur_condense")
        return w, g

    def schur_expand(self, arena, k, w, xt, x=None, stream=None):
        """The full solution x (n doubles, original dof order) from the state w of schur_condense and the caller's solution xt of S x_T = g (m doubles,
        Schur order): cholamd_schur_expand / _f32 by the arena's element type.  w is not modified; x is allocated when None and returned."""
        import torch
        n, m = self.plan.n, self.plan.schur_size(k)
        self._f64_vec(w, "w", n)
        self._f64_vec(xt, "xt", m)
        x = torch.empty(n, dtype=torch.float64, device=f"cuda:{self.device_id}") if x is None else self._f64_vec(x, "x", n)
        fn = self.L.cholamd_schur_expand_f32 if self._is_f32(arena) else self.L.cholamd_schur_expand
        check(fn(self.h, self.ptr(arena), int(k), self.ptr(w), self.ptr(xt), self.ptr(x), _stream_ptr(stream)), "cholamd_schur_expand")
        return x

    def _schur_block(self, t, what, rows, cols=None):
        """_block for an array of `rows` rows; with `cols`: allocate-free check that it has that many columns.  Returns ld."""
        ld, k = self._block(t, what, rows)
        if cols is not None and k != cols:
            raise ValueError(f"{what} has {k} columns, expected {cols}")
        return ld

    def schur_condense_nrhs(self, arena, k, B, W=None, G=None, stream=None):
        """The block form of schur_condense for the columns of B (n x nrhs, column-major, original dof order): W (n x nrhs; column j = the state w of
        column j) and G (m x nrhs, Schur order), allocated when None; returns (W, G).  cholamd_schur_condense_nrhs / _f32 by the arena's element
        type: one pass over the eliminated part of the factor per 32 columns.  Asynchronous on `stream`."""
        import torch
        n, m = self.plan.n, self.plan.schur_size(k)
        ldb, c = self._block(B, "B", n)
        dev = f"cuda:{self.device_id}"
        if W is None:
            W = torch.empty((c, n), dtype=torch.float64, device=dev).T
        if G is None:
            G = torch.empty((c, m), dtype=torch.float64, device=dev).T
        ldw, ldg = self._schur_block(W, "W", n, c), self._schur_block(G, "G", m, c)
        fn = self.L.cholamd_schur_condense_nrhs_f32 if self._is_f32(arena) else self.L.cholamd_schur_condense_nrhs
        check(fn(self.h, self.ptr(arena), int(k), self.ptr(B), ldb, self.ptr(W), ldw, self.ptr(G), ldg, c, _stream_ptr(stream)), "cholamd_schur_condense_nrhs")
        return W, G

    def schur_expand_nrhs(self, arena, k, W, XT, X=None, stream=None):
        """The block form of schur_expand: X (n x nrhs, original dof order; allocated when None, returned) from W of schur_condense_nrhs and the
        caller's XT (m x nrhs, Schur order).  W is not modified.  cholamd_schur_expand_nrhs / _f32 by the arena's element type."""
        import torch
        n, m = self.plan.n, self.plan.schur_size(k)
        ldw, c = self._block(W, "W", n)
        ldxt = self._schur_block(XT, "XT", m, c)
        if X is None:
            X = torch.empty((c, n), dtype=torch.float64, device=f"cuda:{self.device_id}").T
        ldx = self._schur_block(X, "X", n, c)
        fn = self.L.cholamd_schur_expand_nrhs_f32 if self._is_f32(arena) else self.L.cholamd_schur_expand_nrhs
        check(fn(self.h, self.ptr(arena), int(k), self.ptr(W), ldw, self.ptr(XT), ldxt, self.ptr(X), ldx, c, _stream_ptr(stream)), "cholamd_schur_expand_nrhs")
        return X

    def schur_launches(self):
        """Launches of the Schur condense / expand sweeps on this device object so far (cholamd_device_schur_launches): a dict of atomic (the sweep
        kernels that accumulate by atomics), gather and span (the deterministic step lists), copy (the pack / unpack kernels of the block forms)."""
        out = np.zeros(4, dtype=np.int64)
        check(self.L.cholamd_device_schur_launches(self.h, out.ctypes.data), "cholamd_device_schur_launches")
        return dict(zip(("atomic", "gather", "span", "copy"), (int(v) for v in out)))

    def solve_refine_nrhs(self, arena32, B, X, max_iter=20, tol=1e-12, stream=None):
        """cholamd_solve_refine_nrhs: every column of X = A^-1 B by iterative refinement on the fp32 factor; returns (corrections applied, relres per column).
        With the options solve_deterministic and solve_deterministic_block every solve inside is the deterministic block solve: two calls return the
        same corrections, relres and bits (the columns of a chunk of 32 share the number of corrections, so they are not independent of each other)."""
        ldb, ldx, k = self._blocks(B, X)
        it = C.c_int(0)
        rel = np.zeros(max(k, 1), dtype=np.float64)
        check(self.L.cholamd_solve_refine_nrhs(self.h, self.ptr(arena32), self.ptr(B), ldb, self.ptr(X), ldx, k, int(max_iter), float(tol),
                                               C.byref(it), rel.ctypes.data, _stream_ptr(stream)), "cholamd_solve_refine_nrhs")
        return int(it.value), rel[:k]

    # -- y = A x and conjugate gradients preconditioned with the factor at hand (include/cholamd.h at cholamd_solve_pcg) ----------------
    PCG_X0 = 1  # CHOLAMD_PCG_X0

    def apply(self, x, y, stream=None):
        """y = A x with the values in force (cholamd_apply): the fma order of Plan.apply_host; asynchronous; y must not overlap x."""
        check(self.L.cholamd_apply(self.h, self.ptr(x), self.ptr(y), _stream_ptr(stream)), "cholamd_apply")

    def apply_nrhs(self, X, Y, stream=None):
        """Y = A X for the k columns of X (n x k, column-major, as solve_nrhs takes them): cholamd_apply_nrhs."""
        ldx, ldy, k = self._blocks(X, Y)
        check(self.L.cholamd_apply_nrhs(self.h, self.ptr(X), ldx, self.ptr(Y), ldy, k, _stream_ptr(stream)), "cholamd_apply_nrhs")

    def _pcg(self, fn, what, args, k):
        it, st = np.zeros(max(k, 1), dtype=np.int32), np.zeros(max(k, 1), dtype=np.int32)
        rel = np.zeros(max(k, 1), dtype=np.float64)
        rc = fn(*args, it.ctypes.data, rel.ctypes.data, st.ctypes.data)
        try:
            check(rc, what)
        except Exception as e:  # a breakdown (status 2) or NaN (3) in some column: the per-column results travel with the exception
            e.iters, e.relres, e.status = it[:k], rel[:k], st[:k]
            raise
        return it[:k], rel[:k], st[:k]

    def solve_pcg(self, arena, b, x, max_iter=50, tol=1e-12, x0=False, stream=None):
        """A x = b for the values IN FORCE (set_values) by conjugate gradients preconditioned with the factor in `arena` -- the factor of other values
        on the pattern, or an fp32 one (cholamd_solve_pcg / _f32 by the arena's element type).  x0: start from the caller's x instead of zero.  x may
        be b.  Returns (iters, relres, status): applications of A, the true ||b - A x|| / ||b||, 0 converged / 1 max_iter reached.  A breakdown
        (status 2: A or the factor is not positive definite) or NaN (3) raises CholamdError, which carries .iters, .relres and .status."""
        fn = self.L.cholamd_solve_pcg_f32 if self._is_f32(arena) else self.L.cholamd_solve_pcg
        args = (self.h, self.ptr(arena), self.ptr(b), self.ptr(x), int(max_iter), float(tol), self.PCG_X0 if x0 else 0)
        it, rel, st = self._pcg(lambda *a: fn(*a, _stream_ptr(stream)), "cholamd_solve_pcg", args, 1)
        return int(it[0]), float(rel[0]), int(st[0])

    def solve_pcg_nrhs(self, arena, B, X, max_iter=50, tol=1e-12, x0=False, stream=None):
        """The same for the k columns of B (n x k, column-major, as solve_nrhs takes them) in chunks of 32, every column with its own scalars, count
        and status: cholamd_solve_pcg_nrhs / _f32.  Returns the arrays (iters, relres, status).  Under option solve_deterministic a column has the
        bits of solve_pcg on it; with solve_deterministic_block too it depends on its own column of B alone."""
        ldb, ldx, k = self._blocks(B, X)
        fn = self.L.cholamd_solve_pcg_nrhs_f32 if self._is_f32(arena) else self.L.cholamd_solve_pcg_nrhs
        args = (self.h, self.ptr(arena), self.ptr(B), ldb, self.ptr(X), ldx, k, int(max_iter), float(tol), self.PCG_X0 if x0 else 0)
        return self._pcg(lambda *a: fn(*a, _stream_ptr(stream)), "cholamd_solve_pcg_nrhs", args, k)

    def residual(self, b, x, r=None, stream=None):
        """||b - A x|| / ||b|| in fp64 on the device (A = the matrix file's entries)."""
        rel = C.c_double(0.0)
        check(self.L.cholamd_residual(self.h, self.ptr(b), self.ptr(x), self.ptr(r) if r is not None else None, C.byref(rel), _stream_ptr(stream)), "cholamd_residual")
        return rel.value

    def set_timing(self, on):
        check(self.L.cholamd_device_set_timing(self.h, int(on)), "set_timing")

    def event_overhead_ms(self, stream=None):
        v = C.c_float(0)
        check(self.L.cholamd_device_event_overhead(self.h, _stream_ptr(stream), C.byref(v)), "event_overhead")
        return float(v.value)

    def get_timing(self):
        ms = np.zeros(4, dtype=np.float32)
        cnt = np.zeros(4, dtype=np.int32)
        check(self.L.cholamd_device_get_timing(self.h, ms.ctypes.data, cnt.ctypes.data), "get_timing")
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(self.KINDS)}

    def get_timing_ex(self):
        """The compute kinds plus the exchange kinds of a sharded run (cholamd_device_get_timing_ex)."""
        ms = np.zeros(8, dtype=np.float32)
        cnt = np.zeros(8, dtype=np.int32)
        check(self.L.cholamd_device_get_timing_ex(self.h, ms.ctypes.data, cnt.ctypes.data), "get_timing_ex")
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(self.KINDS + ("exchange", "bcast"))}


class Comm:
    """An RCCL communicator owned by libcholamd (cholamd_comm_create: ncclCommInitRank on the device's GPU)."""

    def __init__(self, dev, world, rank, unique_id):
        self.L = load()
        h = C.c_void_p()
        buf = C.create_string_buffer(bytes(unique_id), 128)
        check(self.L.cholamd_comm_create(dev.h, world, rank, buf, C.byref(h)), "cholamd_comm_create")
        self.h, self.world, self.rank = h, world, rank

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        check(load().cholamd_comm_unique_id(buf), "cholamd_comm_unique_id")
        return bytes(buf.raw)

    def count(self):
        """ncclCommCount of the communicator behind the handle."""
        n = C.c_int(0)
        check(self.L.cholamd_comm_count(self.h, C.byref(n)), "cholamd_comm_count")
        return int(n.value)

    def allreduce(self, t, stream=None):
        """In-place fp64 sum of a CUDA tensor over the ranks (cholamd_comm_allreduce)."""
        check(self.L.cholamd_comm_allreduce(self.h, C.c_void_p(t.data_ptr()), t.numel(), _stream_ptr(stream)), "cholamd_comm_allreduce")

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.L.cholamd_comm_destroy(self.h)
                self.h = None
        except Exception:
            pass


def factor_multi(devs, arenas, local=True, streams=None):
    """One process driving the n rank objects `devs` (devs[g] partitioned as rank g of n): cholamd_factor_multi with a LOCAL
    communicator (device-side sums and peer copies: the ranks may share a GPU) or an RCCL one (ncclCommInitAll, one GPU per rank).
    fp32 arenas (torch.float32) take the fp32 schedule (cholamd_factor_multi_f32)."""
    import torch
    L = load()
    f32 = arenas[0].elem_bytes == 4 if isinstance(arenas[0], RankArena) else arenas[0].dtype == torch.float32
    n = len(devs)
    hd = (C.c_void_p * n)(*[d.h for d in devs])
    ha = (C.c_void_p * n)(*[C.c_void_p(a.data_ptr()) for a in arenas])
    hc = (C.c_void_p * n)()
    hs = (C.c_void_p * n)(*[_stream_ptr(s) for s in streams]) if streams is not None else None
    check((L.cholamd_comm_create_local if local else L.cholamd_comm_create_all)(hd, n, hc), "cholamd_comm_create")
    try:
        check((L.cholamd_factor_multi_f32 if f32 else L.cholamd_factor_multi)(hd, ha, hc, n, hs), "cholamd_factor_multi")
        for d in devs:
            d.sync()
    finally:
        for c in hc:
            L.cholamd_comm_destroy(c)


def _multi_call(devs, local, body):
    L = load()
    n = len(devs)
    hd = (C.c_void_p * n)(*[d.h for d in devs])
    hc = (C.c_void_p * n)()
    check((L.cholamd_comm_create_local if local else L.cholamd_comm_create_all)(hd, n, hc), "cholamd_comm_create")
    try:
        out = body(L, n, hd, hc)
        for d in devs:
            d.sync()
        return out
    finally:
        for c in hc:
            L.cholamd_comm_destroy(c)


def solve_multi(devs, arenas, bs, xs, local=True):
    """One process driving the n rank objects through the distributed solve (cholamd_solve_multi): the factor stays where
    cholamd_factor_multi left it, every rank ends with the whole solution in xs[g]."""
    def body(L, n, hd, hc):
        ha = (C.c_void_p * n)(*[C.c_void_p(a.data_ptr()) for a in arenas])
        hb = (C.c_void_p * n)(*[C.c_void_p(b.data_ptr()) for b in bs])
        hx = (C.c_void_p * n)(*[C.c_void_p(x.data_ptr()) for x in xs])
        check(L.cholamd_solve_multi(hd, ha, hb, hx, hc, n, None), "cholamd_solve_multi")
    return _multi_call(devs, local, body)


def solve_refine_multi(devs, arenas32, bs, xs, max_iter=20, tol=1e-12, local=True):
    """cholamd_solve_refine_multi: fp64 refinement with the fp32 factor left on the ranks; returns (corrections, relres)."""
    def body(L, n, hd, hc):
        ha = (C.c_void_p * n)(*[C.c_void_p(a.data_ptr()) for a in arenas32])
        hb = (C.c_void_p * n)(*[C.c_void_p(b.data_ptr()) for b in bs])
        hx = (C.c_void_p * n)(*[C.c_void_p(x.data_ptr()) for x in xs])
        it, rel = C.c_int(0), C.c_double(0.0)
        check(L.cholamd_solve_refine_multi(hd, ha, hb, hx, max_iter, tol, C.byref(it), C.byref(rel), hc, n, None), "cholamd_solve_refine_multi")
        return int(it.value), float(rel.value)
    return _multi_call(devs, local, body)
