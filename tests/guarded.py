"""Guarded caller buffers for the GPU tests (a helper module, not a conftest).

A `Guarded` is an n-vector, or an n x k column-major block with leading dimension ld, inside a torch buffer of G + size + G elements
(size = ld k).  G = 512 elements keeps the view as aligned as a fresh allocation.  The guards and every padding row start as a fixed NaN
bit pattern that the library never computes (0x7FF0DEAD0000BEEF in fp64, 0x7F80BEEF in fp32): a read past the view, or past a column,
brings that NaN into a result, and a write past it changes the pattern.  `assert_guards()` checks that every element outside the data is
still the pattern, bit for bit; `snapshot()` / `assert_unchanged()` check that an input was not written at all."""
import numpy as np

G = 512
PATTERN64 = 0x7FF0DEAD0000BEEF
PATTERN32 = 0x7F80BEEF


class Guarded:
    def __init__(self, rows, cols=None, ld=None, dtype=None, values=None):
        """cols = None: a 1-D view of `rows` elements; else a (rows, cols) view with stride (1, ld).  `values`: the data to start with."""
        import torch
        dtype = torch.float64 if dtype is None else dtype
        self.itype, self.pattern = (torch.int64, PATTERN64) if dtype == torch.float64 else (torch.int32, PATTERN32)
        k = 1 if cols is None else cols
        ld = rows if ld is None else ld
        assert ld >= rows
        self.buf = torch.empty(G + ld * k + G, dtype=dtype, device="cuda")
        self.buf.view(self.itype).fill_(self.pattern)
        body = self.buf[G:G + ld * k].view(k, ld)[:, :rows]
        self.t = body.reshape(rows) if cols is None else body.T
        assert self.t.data_ptr() == self.buf.data_ptr() + G * self.buf.element_size()
        self.data = np.zeros(self.buf.numel(), dtype=bool)    # the elements of the view in the buffer
        self.data[G:G + ld * k].reshape(k, ld)[:, :rows] = True
        if values is not None:
            self.t.copy_(torch.from_numpy(np.asarray(values, dtype=np.float64)).to(dtype))

    def data_ptr(self):
        return self.t.data_ptr()

    def numpy(self):
        """The view as fp64 numpy (a copy)."""
        return self.t.cpu().numpy().astype(np.float64)

    def bits(self):
        return self.buf.view(self.itype).cpu().numpy()

    def assert_guards(self, what=""):
        """Guards and padding rows still hold the pattern, bit for bit."""
        b = self.bits()[~self.data]
        bad = np.nonzero(b != self.pattern)[0]
        assert bad.size == 0, f"{what}: {bad.size} guard / padding elements changed, first at {bad[:4]}"

    def snapshot(self):
        return self.bits().copy()

    def assert_unchanged(self, snap, what=""):
        """The whole buffer -- data, padding and guards -- is bit for bit as in `snap` (an input the library must not write)."""
        bad = np.nonzero(self.bits() != snap)[0]
        assert bad.size == 0, f"{what}: {bad.size} elements of an input changed, first at {bad[:4]}"
