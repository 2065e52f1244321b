"""Reverse mode on the MI355X: the dense adjoints of the R^12 and n = 6 f32 full geometric products against their forward,
gaast_hip_mv_sum_rows against HBM, and the backward of a PGA3D motor sandwich (both VJPs plus sum_rows) against its forward.
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
           "pga3d_sandwich_f32": pga_case(stream, args.steps, args.warmup)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
