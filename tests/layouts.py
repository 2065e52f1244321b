"""Rows of a DeviceMV placed inside a larger, canary-filled torch buffer: the strided, padded and misaligned layouts that
gaast_hip_mv_wrap accepts and that decide, at launch, which row I/O form of a kernel runs.

    p = place(rows, "pad_odd", ga.F32, dim, grades)      # an input: p.mv is the wrapped DeviceMV
    o = place_out(batch, row_len, "shift", ga.F32, dim, grades)
    ... evaluate ...
    p.check()        # the whole buffer, rows and canaries, is bitwise what it was
    o.check()        # every canary before, between and after the rows is untouched
    o.rows()         # [batch, row_len] host array

Strides and shifts are in elements of the dtype.  A plain module, not a conftest.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import gaast_amd as ga
from gaast_amd import _lib
from gaast_amd.graded import _mask_of

NP = {ga.F64: np.float64, ga.F32: np.float32}
BITS = {ga.F64: np.uint64, ga.F32: np.uint32}
CANARY = -777.25          # exactly representable in binary32; no kernel of the library produces it from rows in [-1, 1]
GUARD = 64                # canary elements before the first and after the last row (a multiple of 16 bytes in both types)

# name -> (shift, stride rule); f32 has more ways of missing a 16-byte boundary than f64
LAYOUTS_F64 = ("contig", "pad16", "pad_odd", "shift", "shift_pad16")
LAYOUTS_F32 = LAYOUTS_F64 + ("pad_odd3", "shift2", "shift3")


def layouts_of(dtype):
    return LAYOUTS_F32 if dtype == ga.F32 else LAYOUTS_F64


def geometry(row_len, layout, dtype):
    """(shift, stride) in elements."""
    esz = 8 if dtype == ga.F64 else 4
    per16 = 16 // esz
    pad16 = -(-row_len // per16) * per16 + per16          # next 16-byte multiple, plus one more 16 bytes
    if layout in ("contig", "shared"):
        return 0, row_len
    if layout == "pad16":
        return 0, pad16
    if layout == "pad_odd":
        return 0, row_len + 1
    if layout == "shift":
        return 1, row_len
    if layout == "shift_pad16":
        return 1, pad16
    if dtype == ga.F32:
        if layout == "pad_odd3":
            return 0, row_len + 3
        if layout == "shift2":
            return 2, row_len
        if layout == "shift3":
            return 3, row_len
    raise ValueError(f"no layout {layout!r} for dtype {dtype}")


class Placed:
    def __init__(self, batch, row_len, layout, dtype, dim, grades, rows=None):
        import torch
        ga.init_device()
        self.batch, self.row_len, self.layout, self.dtype = int(batch), int(row_len), layout, dtype
        self.shift, self.stride = geometry(self.row_len, layout, dtype)
        self.esz = 8 if dtype == ga.F64 else 4
        total = GUARD + self.shift + self.batch * self.stride + GUARD
        tdt = torch.float64 if dtype == ga.F64 else torch.float32
        host = np.full(total, CANARY, dtype=NP[dtype])
        self._first = GUARD + self.shift
        idx = (self._first + np.arange(self.batch)[:, None] * self.stride + np.arange(self.row_len)[None, :]).reshape(-1)
        self._row_idx = idx
        self.is_input = rows is not None
        if self.is_input:
            rows = np.ascontiguousarray(rows, dtype=NP[dtype])
            assert rows.shape == (self.batch, self.row_len), (rows.shape, self.batch, self.row_len)
            host[idx] = rows.reshape(-1)
        self.flat = torch.from_numpy(host).to("cuda")
        assert self.flat.data_ptr() % 16 == 0, "torch allocations are expected to be 16-byte aligned"
        self._before = host.view(BITS[dtype]).copy()
        self.ptr = self.flat.data_ptr() + self._first * self.esz
        mask = grades.mask if isinstance(grades, ga.GradeSet) else _mask_of(grades)
        h = C.c_void_p()
        _lib.check(_lib.lib().gaast_hip_mv_wrap(C.c_void_p(self.ptr), dim, mask, self.batch, dtype, self.stride, C.byref(h)))
        self.mv = ga.DeviceMV(h, dim, mask, self.batch, dtype, keep=self.flat)
        assert self.mv.row_len == self.row_len

    # the launch-time rule of runtime.hip (`rows_aligned16`, vector row I/O): base pointer and row stride both multiples of 16 bytes.  A single
    # (shared) row is bound with stride 0.
    def aligned16(self, bound_stride=None):
        stride = self.stride if bound_stride is None else bound_stride
        return self.ptr % 16 == 0 and (stride * self.esz) % 16 == 0

    def _bits(self):
        import torch
        torch.cuda.synchronize()
        _lib.check(_lib.lib().gaast_hip_synchronize())
        return self.flat.cpu().numpy().view(BITS[self.dtype])

    def rows(self):
        return self._bits()[self._row_idx].view(NP[self.dtype]).reshape(self.batch, self.row_len).copy()

    def check(self):
        now = self._bits()
        if self.is_input:
            bad = np.flatnonzero(now != self._before)
            assert bad.size == 0, f"input buffer ({self.layout}) changed at elements {bad[:8]} (first row starts at {self._first}, stride {self.stride})"
            return
        keep = np.ones(now.size, dtype=bool)
        keep[self._row_idx] = False
        bad = np.flatnonzero(keep & (now != self._before))
        assert bad.size == 0, (f"result buffer ({self.layout}): canaries overwritten at elements {bad[:8]} "
                               f"(first row starts at {self._first}, row length {self.row_len}, stride {self.stride}, {self.batch} rows)")


def place(rows, layout, dtype, dim, grades):
    """[batch, row_len] host rows inside a canary-filled device buffer, in `layout`.  layout "shared": one row, batch 1."""
    rows = np.asarray(rows)
    if rows.ndim == 1:
        rows = rows[None, :]
    if layout == "shared":
        assert rows.shape[0] == 1
    return Placed(rows.shape[0], rows.shape[1], layout, dtype, dim, grades, rows=rows)


def place_out(batch, row_len, layout, dtype, dim, grades):
    """a result buffer of `batch` rows in `layout`, rows and gaps filled with the canary"""
    return Placed(batch, row_len, layout, dtype, dim, grades)
