"""The general multivector exponential on the MI355X: one k_mv_gexp<T, N> launch per evaluation and one k_mv_gexp_adj<T, N> launch per
gradient, N = 8 ... 64, f32 and f64.  Prints one JSON line.

Timing as bench.py: inputs resident in HBM, a warm-up, then HIP events on the launch stream around every evaluation.  Operands are
U(-1, 1) normalised to sum |A| = theta (default 3: s = 3 squarings per item).  Per case: the time of a forward evaluation and of a
gradient, items per second, the algorithmic bytes (operand row in, result row out) as a fraction of 8 TB/s, and the forward's
multiply-adds ((m + s) N^2 per item, m = 8 / 14 Horner steps) per second.
    python tools/bench_gexp.py [--steps 20] [--warmup 3] [--batch 1048576] [--theta 3]
"""
import argparse
import ctypes
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before gaast_amd: see tests/conftest.py)

import gaast_amd as ga  # noqa: E402

HBM_BPS = 8.0e12
CASES = [   # name, metric, operand grades, N
    ("R3", [1.0] * 3, [0, 1, 2, 3], 8),
    ("PGA3D-bivector", [0.0, 1.0, 1.0, 1.0], [2], 8),
    ("PGA3D", [0.0, 1.0, 1.0, 1.0], [0, 1, 2, 3, 4], 16),
    ("CGA-bivector", [1.0, 1.0, 1.0, 1.0, -1.0], [2], 16),
    ("CGA", [1.0, 1.0, 1.0, 1.0, -1.0], [0, 1, 2, 3, 4, 5], 32),
    ("R33", [1.0] * 3 + [-1.0] * 3, [0, 1, 2, 3, 4, 5, 6], 64),
]


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


def case(name, metric, grades, N, dtname, batch, theta, stream, steps, warmup):
    dtype = ga.F32 if dtname == "f32" else ga.F64
    tdt = torch.float32 if dtype == ga.F32 else torch.float64
    n = len(metric)
    spec = ga.mv(ga.Input(0, grades, n)).gexp().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    mask, out_len = spec.output_info()
    in_len = sum(int(ga.n_choose_k(n, k)) for k in grades)
    gen = torch.Generator(device="cuda:0").manual_seed(20261019)
    x_t = torch.empty((batch, in_len), device="cuda:0", dtype=tdt).uniform_(-1, 1, generator=gen)
    x_t *= theta / x_t.abs().sum(dim=1, keepdim=True)
    y_t = torch.empty((batch, out_len), device="cuda:0", dtype=tdt)
    g_t = torch.empty((batch, out_len), device="cuda:0", dtype=tdt).uniform_(-1, 1, generator=gen)
    d_t = torch.empty((batch, in_len), device="cuda:0", dtype=tdt)
    x, y = ga.DeviceMV.wrap_tensor(x_t, n, grades), ga.DeviceMV.wrap_tensor(y_t, n, ga.GradeSet(mask))
    g, d = ga.DeviceMV.wrap_tensor(g_t, n, ga.GradeSet(mask)), ga.DeviceMV.wrap_tensor(d_t, n, grades)
    ms = timed(lambda: spec.eval_batch([x], batch, out=y), stream, steps, warmup)
    errors = spec.domain_errors()
    vjp = spec.vjp(0)
    ms_adj = timed(lambda: vjp.eval_batch([x], g, batch, out=d), stream, steps, warmup)
    bytes_ = float(batch) * (in_len + out_len) * x_t.element_size()
    m = 8 if dtype == ga.F32 else 14
    s = max(0, math.ceil(math.log2(theta)) + 1) if theta > 0.5 else 0
    res = {"case": name, "N": N, "dtype": dtname, "batch": batch, "theta": theta, "squarings": s, "launches": spec.launches(), "vjp_launches": vjp.launches(),
           "ms": ms, "items_per_s": batch / ms * 1e3, "GB_s": bytes_ / ms / 1e6, "frac_hbm_8TBs": bytes_ / ms / 1e-3 / HBM_BPS,
           "forward_TFMA_s": float(batch) * (m + s) * N * N / ms / 1e9, "vjp_ms": ms_adj, "vjp_items_per_s": batch / ms_adj * 1e3, "domain_errors": errors}
    del x, y, g, d, x_t, y_t, g_t, d_t, spec, vjp
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--theta", type=float, default=3.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gexp.py measures on the GPU: no device visible")
    ga.init_device()
    stream = torch.cuda.current_stream()
    ga._lib.check(ga.lib().gaast_hip_set_stream(ctypes.c_void_p(stream.cuda_stream)))
    out = []
    for name, metric, grades, N in CASES:
        for dtname in ("f32", "f64"):
            out.append(case(name, metric, grades, N, dtname, args.batch, args.theta, stream, args.steps, args.warmup))
    print(json.dumps({"bench": "gexp", "device": torch.cuda.get_device_name(0), "cases": out}))


if __name__ == "__main__":
    main()
