"""torch binding with reverse mode: `spec.torch_fn()` is a callable on torch tensors backed by a torch.autograd.Function.

Every argument is a contiguous f32 / f64 GPU tensor [B or 1, row_len] in the layout of its input slot (the spec's dtype; a batch-1
tensor is shared by every item).  Forward evaluates the program, backward its VJP programs (gaast_program_vjp): one per input that
needs a gradient, built on first use and kept by the spec.  The gradient of a shared (batch-1) input among batch-B inputs is the sum
of its per-item gradients (gaast_hip_mv_sum_rows).  Both directions run on torch's current stream.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .grade_set import GradeSet
from .graded import DeviceMV, row_len

_TORCH_DTYPE = {_lib.F64: torch.float64, _lib.F32: torch.float32}


def _wrap(t, dim, mask):
    return DeviceMV.wrap_tensor(t, dim, GradeSet(mask))


def _use_torch_stream():
    _lib.init_device()
    _lib.check(_lib.lib().gaast_hip_set_stream(C.c_void_p(torch.cuda.current_stream().cuda_stream)))


class _ProgramFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, spec, layouts, *xs):
        want = _TORCH_DTYPE[spec.dtype]
        B = 1
        for i, x in enumerate(xs):
            if x.dtype != want:
                raise TypeError(f"input {i}: {x.dtype}, but the program was specialised for {want}")
            dim, mask = layouts[i]
            if x.dim() != 2 or x.shape[1] != row_len(dim, mask):
                raise ValueError(f"input {i}: expected [B or 1, {row_len(dim, mask)}], got {list(x.shape)}")
            if x.shape[0] != 1:
                if B != 1 and x.shape[0] != B:
                    raise ValueError(f"input {i}: batch {x.shape[0]} differs from {B}")
                B = x.shape[0]
        xs = tuple(x.contiguous() for x in xs)
        _use_torch_stream()
        mask, rl = spec.output_info()
        out = torch.empty((B, rl), dtype=want, device=xs[0].device if xs else "cuda")
        ins = [_wrap(x, *layouts[i]) for i, x in enumerate(xs)]
        spec.eval_batch(ins, B, out=_wrap(out, spec.get_node(spec.root_id()).vec_space_dim, mask))
        ctx.spec, ctx.layouts, ctx.batch = spec, layouts, B
        ctx.out_layout = (spec.get_node(spec.root_id()).vec_space_dim, mask)
        ctx.save_for_backward(*xs)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        xs = ctx.saved_tensors
        spec, B = ctx.spec, ctx.batch
        g = g.contiguous()
        _use_torch_stream()
        ins = [_wrap(x, *ctx.layouts[i]) for i, x in enumerate(xs)]
        cot = _wrap(g, *ctx.out_layout)
        grads = [None, None]
        for i, x in enumerate(xs):
            if not ctx.needs_input_grad[i + 2]:
                grads.append(None)
                continue
            dim, mask = ctx.layouts[i]
            v = spec.vjp(i)
            per_item = torch.empty((B, x.shape[1]), dtype=x.dtype, device=x.device)
            pm = v.eval_batch(ins, cot, B, out=_wrap(per_item, dim, mask))
            if x.shape[0] == 1 and B > 1:
                total = torch.empty((1, x.shape[1]), dtype=x.dtype, device=x.device)
                pm.sum_rows(_wrap(total, dim, mask))
                grads.append(total)
            else:
                grads.append(per_item)
        return tuple(grads)


def torch_fn(spec):
    """f(*tensors) -> output tensor [B, out_row_len], differentiable in every input slot of `spec`."""
    d = spec.program_desc()
    layouts = tuple((d.inputs[i].storage_dim, d.inputs[i].grade_mask) for i in range(spec.num_user_inputs()))

    def fn(*xs):
        if len(xs) != len(layouts):
            raise TypeError(f"expected {len(layouts)} tensors, got {len(xs)}")
        return _ProgramFunction.apply(spec, layouts, *xs)

    return fn


class _OutermorphismFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dtype, dim, mask, m, rows):
        want = _TORCH_DTYPE[dtype]
        if m.dtype != want or rows.dtype != want:
            raise TypeError(f"M and rows must be {want}")
        if tuple(m.shape) != (dim, dim):
            raise ValueError(f"M: expected [{dim}, {dim}], got {list(m.shape)}")
        if rows.dim() != 2 or rows.shape[1] != row_len(dim, mask):
            raise ValueError(f"rows: expected [B, {row_len(dim, mask)}], got {list(rows.shape)}")
        from .graded import Outermorphism
        rows = rows.contiguous()
        _use_torch_stream()
        om = Outermorphism(m.detach().cpu().numpy(), dtype)   # the download synchronises: compounds are built on the host
        out = torch.empty_like(rows)
        om.apply(_wrap(rows, dim, mask), out=_wrap(out, dim, mask))
        ctx.om, ctx.dim, ctx.mask = om, dim, mask
        ctx.save_for_backward(rows)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (rows,) = ctx.saved_tensors
        om, dim, mask = ctx.om, ctx.dim, ctx.mask
        g = g.contiguous()
        _use_torch_stream()
        cot = _wrap(g, dim, mask)
        dm = drows = None
        if ctx.needs_input_grad[3]:
            dm = om.matrix_vjp(_wrap(rows, dim, mask), cot, out=torch.empty((dim, dim), dtype=rows.dtype, device=rows.device))
        if ctx.needs_input_grad[4]:
            drows = torch.empty_like(rows)
            om.apply_transposed(cot, out=_wrap(drows, dim, mask))
        return None, None, None, dm, drows


def outermorphism_fn(dtype=_lib.F64):
    """f(M, rows, dim, grades) -> rows mapped by the outermorphism of M (C_k(M) on grade k), differentiable in M and in the rows.

    M: an [n, n] GPU tensor, rows: [B, row_len] in the layout of (dim, grades), both of `dtype`.  Forward DOWNLOADS M -- a
    synchronisation of the current stream -- because the compounds of a linear map are built on the host (gaast_hip_linmap_create),
    then creates the map and applies it.  Backward returns gaast_hip_linmap_matrix_vjp for M (n <= 8) and
    gaast_hip_linmap_apply_transposed for the rows.  Both directions run on torch's current stream.  No double backward."""

    def fn(m, rows, dim, grades):
        mask = grades.mask if isinstance(grades, GradeSet) else sum(1 << int(k) for k in set(grades))
        return _OutermorphismFunction.apply(dtype, int(dim), mask, m, rows)

    return fn
