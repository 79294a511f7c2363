"""Differentiable solve and log det: torch.autograd on top of the factor, the block solve, the selected inversion and the values-gradient kernels.

    fac = factorize(dev, values)            # values: the value array of Device.set_values, a CUDA tensor that may require grad
    loss = (T * fac.solve(B)).sum() + c * fac.logdet()
    loss.backward()                         # values.grad, B.grad

A(v) = sum_k v_k E_k is the matrix of the plan's pattern with the value array v (include/cholamd.h at cholamd_values_grad_pairs).  A is symmetric, so the
adjoint of X = A^-1 B is one more block solve, Lam = A^-1 dloss/dX; then dloss/dB = Lam and dloss/dv_k = -sum_c lam_c^T E_k x_c, which
Device.values_grad_pairs contracts onto the value array.  d(log det A)/dv_k = tr(A^-1 E_k) comes from the selected inverse (Device.selinv, once per
Factorization) through Device.values_grad_logdet.  Every numeric step is a call into libcholamd.so on torch's current stream; nothing here computes on the
CPU.  fp64 factor of a single GPU; no double backward.

A Factorization is FIXED at the values it was built from: after a change of the values (an optimiser step) call factorize again -- nothing detects a
stale factor.  The device object's buffers are its own, so one Factorization per device object is in use at a time (factorize on the same `dev`
refills the same scatter list)."""
import torch
from torch.autograd.function import once_differentiable

from ._lib import CholamdError


def _stream(dev):
    return torch.cuda.current_stream(dev.device_id)


def _colmajor(dev, src, k):
    """A fresh n x k column-major block (stride (1, n)) holding `src` (n x k, any strides)."""
    out = torch.empty((k, dev.plan.n), dtype=torch.float64, device=f"cuda:{dev.device_id}").T
    out.copy_(src)
    return out


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, B, fac):
        dev = fac.dev
        k = 1 if B.dim() == 1 else B.shape[1]
        Bc = _colmajor(dev, B.detach().reshape(dev.plan.n, k), k)
        X = torch.empty((k, dev.plan.n), dtype=torch.float64, device=B.device).T
        dev.solve_nrhs(fac.arena, Bc, X, stream=_stream(dev))
        out = X[:, 0] if B.dim() == 1 else X
        ctx.fac = fac
        ctx.save_for_backward(out)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_X):
        fac, dev = ctx.fac, ctx.fac.dev
        X, = ctx.saved_tensors
        one_d = X.dim() == 1
        X = X.unsqueeze(1) if one_d else X
        k = X.shape[1]
        need_values, need_B = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_values or need_B):
            return None, None, None
        st = _stream(dev)
        G = _colmajor(dev, grad_X.reshape(dev.plan.n, k), k)
        Lam = torch.empty((k, dev.plan.n), dtype=torch.float64, device=X.device).T
        dev.solve_nrhs(fac.arena, G, Lam, stream=st)
        grad_values = dev.values_grad_pairs(Lam, X, alpha=-1.0, beta=0.0, stream=st) if need_values else None
        grad_B = (Lam[:, 0] if one_d else Lam) if need_B else None
        return grad_values, grad_B, None


class _LogDet(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, fac):
        dev = fac.dev
        ctx.fac = fac
        return torch.tensor(dev.logdet(fac.arena, stream=_stream(dev)), dtype=torch.float64, device=f"cuda:{dev.device_id}")

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        fac, dev = ctx.fac, ctx.fac.dev
        if not ctx.needs_input_grad[0]:
            return None, None
        st = _stream(dev)
        if fac._z is None:
            fac._z = dev.selinv(fac.arena, stream=st)
        g = dev.values_grad_logdet(fac._z, alpha=1.0, beta=0.0, stream=st)
        return g.mul_(grad), None  # the incoming scalar stays on the device: no synchronisation for it


class Factorization:
    """The fp64 factor of A(values) in an arena, with differentiable solve() and logdet() (see the module docstring).  Made by factorize()."""

    def __init__(self, dev, values, arena):
        self.dev, self.values, self.arena = dev, values, arena
        self._z = None  # the Z arena of the selected inversion, computed by the first backward pass of a logdet()

    def _check_B(self, B):
        n = self.dev.plan.n
        if not isinstance(B, torch.Tensor) or B.dtype != torch.float64 or not B.is_cuda or B.device.index != self.dev.device_id:
            raise ValueError(f"B must be a float64 tensor on cuda:{self.dev.device_id}")
        if B.dim() not in (1, 2) or B.shape[0] != n:
            raise ValueError(f"B must have shape (n,) or (n, nrhs) with n = {n}; got {tuple(B.shape)}")

    def solve(self, B):
        """X = A^-1 B for B of shape (n,) or (n, nrhs), float64 on the factor's GPU, any strides (torch's row-major (n, nrhs) is copied into the
        column-major block Device.solve_nrhs takes); X has B's shape.  Differentiable with respect to `values` and B."""
        self._check_B(B)
        if B.dim() == 2 and B.shape[1] == 0:
            return B.new_empty(B.shape)
        return _Solve.apply(self.values, B, self)

    def logdet(self):
        """log det A as a 0-dim float64 tensor on the factor's GPU (Device.logdet: synchronises the current stream).  Differentiable with respect to
        `values`; the first backward pass runs the selected inversion and keeps its Z arena on this object (release() drops it)."""
        return _LogDet.apply(self.values, self)

    def release(self):
        """Drop the Z arena of the selected inversion (a second arena's worth of device memory); the next logdet backward computes it again."""
        self._z = None


def factorize(dev, values, arena=None):
    """Factor A(values) on `dev` (a single-GPU Device): set_values(check=True), fill, factor, info() on torch's current stream.  `values`: a contiguous
    1-D float64 CUDA tensor of plan.nz elements in the order of plan.entries(); it may require grad.  `arena`: the fp64 arena to factor in (a tensor of
    Device.new_arena()'s size); allocated when None.  Raises CholamdError when a pivot fails (the matrix is not positive definite) or when the value
    array gives an entry outside the pattern a non-zero value; ValueError for a value array of the wrong kind."""
    if not isinstance(values, torch.Tensor):
        raise ValueError("values must be a contiguous 1-D float64 CUDA tensor (the tensor to differentiate with respect to)")
    if arena is None:
        arena = dev.new_arena()
    elif not isinstance(arena, torch.Tensor) or arena.dtype != torch.float64 or not arena.is_cuda or arena.numel() != dev.plan.arena_doubles or not arena.is_contiguous():
        raise ValueError(f"arena must be a contiguous float64 CUDA tensor of plan.arena_doubles = {dev.plan.arena_doubles} elements")
    st = _stream(dev)
    dev.set_values(values.detach(), check=True, stream=st)
    dev.fill(arena, stream=st)
    dev.factor(arena, stream=st)
    dev.sync(st)
    info, sep = dev.info()
    if info != 0:
        raise CholamdError(f"factorize: the matrix is not positive definite: pivot {info} failed (separator {sep})")
    return Factorization(dev, values, arena)
