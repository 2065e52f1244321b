"""Reverse mode on the MI355X: the dense adjoints of the R^12 and n = 6 f32 full geometric products against their forward,
gaast_hip_mv_sum_rows against HBM, the backward of a PGA3D motor sandwich (both VJPs plus sum_rows) against its forward, and
rotor_grad: the PGA3D sandwich exp(B) X ~exp(B) differentiated through exp (GAAST_FLAG_EXP_LOG | GAAST_FLAG_EXP_LOG_GRAD) with a
shared and with a batched generator, plus the stand-alone adjoint kernel k_exp_log_adj against HBM at m = 6 and m = 66 components.
Prints one JSON line.

Timing as bench.py: inputs resident in HBM, a warm-up, then HIP events on the launch stream around every call.
    python tools/bench_vjp.py [--steps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before gaast_amd: see tests/conftest.py)

import gaast_amd as ga  # noqa: E402

HBM_BPS = 8.0e12


def timed(fn, stream, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for e0, e1 in evs:
        e0.record(stream)
        fn()
        e1.record(stream)
    torch.cuda.synchronize()
    return sum(e0.elapsed_time(e1) for e0, e1 in evs) / steps


def rows(batch, n_comp):
    return torch.empty((batch, n_comp), device="cuda:0", dtype=torch.float32).uniform_(-1, 1)


def gp_case(n, batch, stream, steps, warmup):
    full = list(range(n + 1))
    spec = (ga.mv(ga.Input(0, full, n)) * ga.mv(ga.Input(1, full, n))).specialize(n, dtype=ga.F32)
    ts = [rows(batch, 1 << n) for _ in range(3)]
    a, b, g = (ga.DeviceMV.wrap_tensor(t, n, full) for t in ts)
    o_t = rows(batch, 1 << n)
    o = ga.DeviceMV.wrap_tensor(o_t, n, full)
    res = {"n": n, "batch": batch, "forward_ms": timed(lambda: spec.eval_batch([a, b], batch, out=o), stream, steps, warmup),
           "forward_launches": spec.launches()}
    for slot in range(2):
        v = spec.vjp(slot)
        res[f"vjp{slot}_ms"] = timed(lambda: v.eval_batch([a, b], g, batch, out=o), stream, steps, warmup)
        res[f"vjp{slot}_launches"] = v.launches()
        res[f"vjp{slot}_over_forward"] = res[f"vjp{slot}_ms"] / res["forward_ms"]
    return res


def sum_rows_case(batch, n_comp, dim, grades, stream, steps, warmup):
    x_t = rows(batch, n_comp)
    x = ga.DeviceMV.wrap_tensor(x_t, dim, grades)
    out = ga.DeviceMV.alloc(dim, grades, 1, ga.F32)
    ms = timed(lambda: x.sum_rows(out), stream, steps, warmup)
    bytes_ = batch * n_comp * 4.0
    return {"batch": batch, "row": n_comp, "MB": bytes_ / 1e6, "ms": ms, "GB_s": bytes_ / ms / 1e6, "frac_hbm_8TBs": bytes_ / ms / 1e-3 / HBM_BPS}


def pga_case(stream, steps, warmup, batch=1 << 20):
    n, metric = 4, [0.0, 1.0, 1.0, 1.0]
    M, X = ga.mv(ga.Input(0, [0, 2, 4], n)), ga.mv(ga.Input(1, [3], n))
    spec = (M * X * M.rev()).specialize(metric, dtype=ga.F32)
    f = spec.torch_fn()
    m_t = rows(1, 8).requires_grad_()
    x_t = rows(batch, 4).requires_grad_()
    y = f(m_t, x_t)
    gy = torch.ones_like(y)
    fwd = timed(lambda: f(m_t, x_t), stream, steps, warmup)

    def backward():
        torch.autograd.grad(y, (m_t, x_t), gy, retain_graph=True)
    bwd = timed(backward, stream, steps, warmup)
    return {"batch": batch, "forward_ms": fwd, "backward_ms": bwd, "backward_over_forward": bwd / fwd}


def rotor_grad_case(shared, stream, steps, warmup, batch=1 << 20):
    """PGA3D exp(B) X ~exp(B), f32: forward, backward (both VJPs, + sum_rows when B is shared), launches per backward"""
    n, metric = 4, [0.0, 1.0, 1.0, 1.0]
    R = ga.mv(ga.Input(0, [2], n)).exp()
    spec = (R * ga.mv(ga.Input(1, [3], n)) * R.rev()).g(3).specialize(metric, dtype=ga.F32, flags=ga.FLAG_EXP_LOG | ga.FLAG_EXP_LOG_GRAD)
    f = spec.torch_fn()
    b_t = rows(1 if shared else batch, 6).mul_(0.5).requires_grad_()
    x_t = rows(batch, 4).requires_grad_()
    y = f(b_t, x_t)
    gy = torch.ones_like(y)
    fwd = timed(lambda: f(b_t, x_t), stream, steps, warmup)
    bwd = timed(lambda: torch.autograd.grad(y, (b_t, x_t), gy, retain_graph=True), stream, steps, warmup)
    launches = [len(spec.vjp(s).launches()) for s in range(2)]
    return {"batch": batch, "shared_generator": shared, "forward_ms": fwd, "backward_ms": bwd, "backward_over_forward": bwd / fwd,
            "forward_launches": len(spec.launches()), "vjp_launches": launches,
            "launches_per_backward": sum(launches) + (1 if shared else 0)}


def cga_sandwich_case(stream, steps, warmup, batch=1 << 20):
    """conformal R X ~R (R: grades {0, 2}, shared; X: points), f32: backward against forward in the null basis {e1, e2, e3, e_o,
    e_inf} (Gram metric: linmap launches around the program) and the same program in the diagonal basis (+ + + + -), alternating"""
    n = 5
    null = np.array([[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, -1], [0, 0, 0, -1, 0]], dtype=np.float64)
    out = {"batch": batch}
    cases = {}
    for name, alg in (("null_basis", ga.GramAlgebra(null)), ("diagonal_basis", ga.MetricAlgebra([1.0, 1.0, 1.0, 1.0, -1.0]))):
        R, X = ga.mv(ga.Input(0, [0, 2], n)), ga.mv(ga.Input(1, [1], n))
        spec = (R * X * R.rev()).g(1).specialize(alg, dtype=ga.F32)
        f = spec.torch_fn()
        r_t, x_t = rows(1, 11).requires_grad_(), rows(batch, 5).requires_grad_()
        y = f(r_t, x_t)
        cases[name] = (spec, f, r_t, x_t, y, torch.ones_like(y))
        out[name] = {"forward_ms": [], "backward_ms": [], "forward_launches": len(spec.launches()),
                     "vjp_launches": [len(spec.vjp(s).launches()) for s in range(2)]}
    for _ in range(3):
        for name, (spec, f, r_t, x_t, y, gy) in cases.items():
            out[name]["forward_ms"].append(timed(lambda: f(r_t, x_t), stream, steps, warmup))
            out[name]["backward_ms"].append(timed(lambda: torch.autograd.grad(y, (r_t, x_t), gy, retain_graph=True), stream, steps, warmup))
    for name in cases:
        out[name]["backward_over_forward"] = min(out[name]["backward_ms"]) / min(out[name]["forward_ms"])
    out["null_over_diagonal_backward"] = min(out["null_basis"]["backward_ms"]) / min(out["diagonal_basis"]["backward_ms"])
    return out


def exp_adj_kernel_case(n, stream, steps, warmup, batch):
    """k_exp_log_adj alone on R^n bivectors, f32.  The unfused (NO_FUSION) VJP of exp(B) is the copies of B and g into their cache
    buffers, the zero fill of the result and the adjoint launch; the two copies are timed as programs of their own (an input as the
    root: zero fill + add_grades_from over the same rows) and subtracted.  HBM fraction from the rows the kernel moves: B and g
    read, the gradient row read and written."""
    m = n * (n - 1) // 2
    grad = ga.FLAG_EXP_LOG | ga.FLAG_EXP_LOG_GRAD | ga.FLAG_NO_FUSION
    v = ga.mv(ga.Input(0, [2], n)).exp().specialize(n, dtype=ga.F32, flags=grad).vjp(0)
    b = ga.DeviceMV.wrap_tensor(rows(batch, m).mul_(0.2), n, [2])
    g = ga.DeviceMV.wrap_tensor(rows(batch, m + 1), n, [0, 2])
    o = ga.DeviceMV.wrap_tensor(rows(batch, m), n, [2])
    o_g = ga.DeviceMV.wrap_tensor(rows(batch, m + 1), n, [0, 2])
    copy_b = ga.mv(ga.Input(0, [2], n)).specialize(n, dtype=ga.F32, flags=ga.FLAG_NO_FUSION)
    copy_g = ga.mv(ga.Input(0, [0, 2], n)).specialize(n, dtype=ga.F32, flags=ga.FLAG_NO_FUSION)
    plan_ms = timed(lambda: v.eval_batch([b], g, batch, out=o), stream, steps, warmup)
    copies_ms = timed(lambda: copy_b.eval_batch([b], batch, out=o), stream, steps, warmup) + \
        timed(lambda: copy_g.eval_batch([g], batch, out=o_g), stream, steps, warmup)
    kernel_ms = plan_ms - copies_ms
    moved = (m + (m + 1) + 2 * m) * 4.0 * batch
    return {"n": n, "m": m, "batch": batch, "launches": v.launches(), "copy_launches": copy_b.launches() + copy_g.launches(),
            "plan_ms": plan_ms, "copies_ms": copies_ms, "kernel_ms": kernel_ms, "kernel_bytes": moved,
            "kernel_frac_hbm_8TBs": moved / (kernel_ms * 1e-3) / HBM_BPS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    ga.init_device(0)
    stream = torch.cuda.current_stream()
    ga.lib().gaast_hip_set_stream(torch.cuda.current_stream().cuda_stream)
    out = {"metric": "reverse mode: dense adjoints vs forward, sum_rows vs HBM, PGA3D sandwich backward vs forward",
           "r12_f32": gp_case(12, 65536, stream, args.steps, args.warmup),
           "n6_f32": gp_case(6, 1 << 22, stream, args.steps, args.warmup),
           "sum_rows_f32_row16": sum_rows_case(1 << 22, 16, 16, [1], stream, args.steps, args.warmup),
           "sum_rows_f32_row8": sum_rows_case(1 << 23, 8, 8, [1], stream, args.steps, args.warmup),
           "sum_rows_f32_row4096": sum_rows_case(1 << 14, 4096, 12, list(range(13)), stream, args.steps, args.warmup),
           "pga3d_sandwich_f32": pga_case(stream, args.steps, args.warmup),
           "rotor_grad_shared_f32": rotor_grad_case(True, stream, args.steps, args.warmup),
           "rotor_grad_batched_f32": rotor_grad_case(False, stream, args.steps, args.warmup),
           "cga_null_basis_sandwich_f32": cga_sandwich_case(stream, args.steps, args.warmup),
           "exp_adj_kernel_m6_f32": exp_adj_kernel_case(4, stream, args.steps, args.warmup, 1 << 22),
           "exp_adj_kernel_m66_f32": exp_adj_kernel_case(12, stream, args.steps, args.warmup, 1 << 19)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
