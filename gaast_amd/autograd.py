"""torch binding with reverse mode: `spec.torch_fn()` is a callable on torch tensors backed by a torch.autograd.Function.

Every argument is a contiguous f32 / f64 GPU tensor [B or 1, row_len] in the layout of its input slot (the spec's dtype; a batch-1
tensor is shared by every item).  Forward evaluates the program, backward its VJP programs (gaast_program_vjp): one per input that
needs a gradient, built on first use and kept by the spec.  The gradient of a shared (batch-1) input among batch-B inputs is the sum
of its per-item gradients (gaast_hip_mv_sum_rows).  Both directions run on torch's current stream.

Backward is differentiable to any order (create_graph=True: Hessian-vector products, gradient penalties): each gradient is a second
autograd.Function over the Vjp object, whose own backward evaluates Vjp.vjp(slot), built when first asked for.  Programs that hold
exp / log / gexp / gsqrt / glog on the path differentiate once; asking for their second derivative raises GaastError UNIMPLEMENTED --
except through gexp on a spec built with specialize(..., flags=FLAG_GEXP_GRAD2): there second order (and forward mode, spec.jvp)
works, and it is the third order that is refused.  With FLAG_GSQRT_GLOG_JVP every order works through gsqrt, and forward mode
(spec.jvp) through glog; a second derivative with respect to an input under glog needs FLAG_GSQRT_GLOG_JVP | FLAG_GLOG_GRAD2: then
create_graph=True gives Hessian-vector products and gradient penalties through glog (third order is refused).  exp / log are unchanged.
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
    def backward(ctx, g):
        xs = ctx.saved_tensors
        g = g.contiguous()
        grads = [None, None]
        for i in range(len(xs)):
            grads.append(_gradient(ctx.spec, i, xs, g, ctx.batch) if ctx.needs_input_grad[i + 2] else None)
        return tuple(grads)


def _bound_slots(prog):
    """The slots of `prog` (a SpecializedAst or a Vjp) that tensors are bound to, in the order of the tensors."""
    if hasattr(prog, "parent"):
        return _bound_slots(prog.parent) + [prog.n_fwd]
    return list(range(prog.num_user_inputs()))


def _gradient(prog, k, ts, cot, B):
    """The gradient of <cot, prog(*ts)> with respect to ts[k]: one row per item, or their sum for a shared (batch-1) tensor among
    B items.  Differentiable when grad mode is on (backward under create_graph=True); the VJP program is built on first use."""
    v = prog.vjp(_bound_slots(prog)[k])
    per_item = _VjpFunction.apply(v, B, *ts, cot)
    if ts[k].shape[0] == 1 and B > 1:
        return _SumRowsFunction.apply(per_item, v.wrt_dim, v.wrt_mask)
    return per_item


class _VjpFunction(torch.autograd.Function):
    """The per-item gradient rows of a Vjp object as a function of its bound tensors (those of the program it differentiates,
    then the cotangent).  Its own backward evaluates Vjp.vjp(slot) through this same class, so any order differentiates."""

    @staticmethod
    def forward(ctx, v, B, *ts):
        _use_torch_stream()
        d = v.desc
        slots = _bound_slots(v)
        ins = [_wrap(t, d.inputs[s].storage_dim, d.inputs[s].grade_mask) for s, t in zip(slots, ts)]
        per_item = torch.empty((B, row_len(v.wrt_dim, v.wrt_mask)), dtype=ts[-1].dtype, device=ts[-1].device)
        v.eval_batch(ins[:-1], ins[-1], B, out=_wrap(per_item, v.wrt_dim, v.wrt_mask))
        ctx.v, ctx.batch = v, B
        ctx.save_for_backward(*ts)
        return per_item

    @staticmethod
    def backward(ctx, h):
        ts = ctx.saved_tensors
        # the cotangent of a summed gradient arrives as a stride-0 expansion of one row: a batch-1 tensor binds as shared
        h = h[:1].contiguous() if h.shape[0] > 1 and h.stride(0) == 0 else h.contiguous()
        grads = [None, None]
        for k in range(len(ts)):
            grads.append(_gradient(ctx.v, k, ts, h, ctx.batch) if ctx.needs_input_grad[k + 2] else None)
        return tuple(grads)


class _SumRowsFunction(torch.autograd.Function):
    """gaast_hip_mv_sum_rows: the reduction of the per-item gradients of a shared input.  Linear: its backward hands the one-row
    cotangent to every item, as a stride-0 expansion that is bound as a shared input again (no expansion kernel)."""

    @staticmethod
    def forward(ctx, per_item, dim, mask):
        _use_torch_stream()
        total = torch.empty((1, per_item.shape[1]), dtype=per_item.dtype, device=per_item.device)
        _wrap(per_item, dim, mask).sum_rows(_wrap(total, dim, mask))
        ctx.batch = per_item.shape[0]
        return total

    @staticmethod
    def backward(ctx, h):
        return h.expand(ctx.batch, h.shape[1]), None, None


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
