"""The general multivector logarithm on the MI355X: one k_mv_glog<T, N> launch per evaluation and one k_mv_glog_adj<T, N> launch per
gradient, N = 8 ... 64, f32 and f64.  Prints one JSON line.

Timing as bench.py: inputs resident in HBM, a warm-up, then HIP events on the launch stream around every evaluation.  Operands have a
principal logarithm by construction: A = gexp(B), computed on the GPU by the library's own gexp, B = U(-1, 1) normalised to
sum |B| = theta (default 1: two or three roots).  Per case: the time of a forward evaluation and of a gradient, items per second, the
algorithmic bytes (operand row in, result row out) as a fraction of 8 TB/s, the roots s and the root steps k the numpy restatement
(tests/glog_numpy.py, tests/gsqrt_numpy.py) takes on the first 64 items, and the forward's multiply-adds (k (N^3 / 2 + N^2) per item
for the roots: an elimination and a product per step; 7 N^3 / 2 for the Pade solves) per second with their share of the vector FMA
peak (78.6 T/s in f32, 39.3 T/s in f64).
    python tools/bench_glog.py [--steps 20] [--warmup 3] [--batch 1048576] [--theta 1]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before gaast_amd: see tests/conftest.py)

import numpy as np  # noqa: E402

import gaast_amd as ga  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import glog_numpy as gl  # noqa: E402  (the numpy restatement: how many roots and root steps the items take)
import gsqrt_numpy as gs  # noqa: E402

HBM_BPS = 8.0e12
FMA_PEAK = {"f32": 78.6e12, "f64": 39.3e12}
CASES = [   # name, metric, grades of the generator B, N
    ("R3", [1.0] * 3, [0, 1, 2, 3], 8),
    ("PGA3D-even", [0.0, 1.0, 1.0, 1.0], [2], 8),
    ("PGA3D", [0.0, 1.0, 1.0, 1.0], [0, 1, 2, 3, 4], 16),
    ("CGA-even", [1.0, 1.0, 1.0, 1.0, -1.0], [2], 16),
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
    make = ga.mv(ga.Input(0, grades, n)).gexp().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    mask, row_len = make.output_info()
    sgrades = [k for k in range(n + 1) if (mask >> k) & 1]        # the grades of the blade set: the logarithm's operand and its result
    spec = ga.mv(ga.Input(0, sgrades, n)).glog().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    assert spec.output_info() == (mask, row_len)
    in_len = sum(int(ga.n_choose_k(n, k)) for k in grades)
    gen = torch.Generator(device="cuda:0").manual_seed(20261021)
    b_t = torch.empty((batch, in_len), device="cuda:0", dtype=tdt).uniform_(-1, 1, generator=gen)
    b_t *= theta / b_t.abs().sum(dim=1, keepdim=True)
    x_t = torch.empty((batch, row_len), device="cuda:0", dtype=tdt)
    y_t = torch.empty((batch, row_len), device="cuda:0", dtype=tdt)
    g_t = torch.empty((batch, row_len), device="cuda:0", dtype=tdt).uniform_(-1, 1, generator=gen)
    d_t = torch.empty((batch, row_len), device="cuda:0", dtype=tdt)
    sset = ga.GradeSet(mask)
    x, y = ga.DeviceMV.wrap_tensor(x_t, n, sset), ga.DeviceMV.wrap_tensor(y_t, n, sset)
    g, d = ga.DeviceMV.wrap_tensor(g_t, n, sset), ga.DeviceMV.wrap_tensor(d_t, n, sset)
    make.eval_batch([ga.DeviceMV.wrap_tensor(b_t, n, grades)], batch, out=x)      # A = gexp(B)
    torch.cuda.synchronize()
    ms = timed(lambda: spec.eval_batch([x], batch, out=y), stream, steps, warmup)
    errors = spec.domain_errors()
    vjp = spec.vjp(0)
    ms_adj = timed(lambda: vjp.eval_batch([x], g, batch, out=d), stream, steps, warmup)
    sample = x_t[:64].cpu().numpy()
    import gexp_numpy as gx
    npdt = np.float32 if dtype == ga.F32 else np.float64
    X = gx.to_s(metric, sgrades, sample)
    roots = gl.forward(metric, sgrades, X, npdt)[1]
    k = np.zeros(len(X))
    for _ in range(int(roots.max())):                               # the steps of every root an item takes
        go = roots > 0
        Xr, st, _ = gs.forward(metric, sgrades, X[go], npdt)
        X[go] = Xr
        k[go] += st
        roots = roots - go
    roots = gl.forward(metric, sgrades, gx.to_s(metric, sgrades, sample), npdt)[1]
    bytes_ = float(batch) * 2 * row_len * x_t.element_size()
    fma = float(batch) * (float(k.mean()) * (N ** 3 / 2 + N * N) + 7 * N ** 3 / 2)
    res = {"case": name, "N": N, "dtype": dtname, "batch": batch, "theta": theta, "roots_mean": float(roots.mean()), "roots_max": int(roots.max()),
           "root_steps_mean": float(k.mean()), "root_steps_max": int(k.max()),
           "launches": spec.launches(), "vjp_launches": vjp.launches(),
           "ms": ms, "items_per_s": batch / ms * 1e3, "GB_s": bytes_ / ms / 1e6, "frac_hbm_8TBs": bytes_ / ms / 1e-3 / HBM_BPS,
           "forward_TFMA_s": fma / ms / 1e9, "frac_fma_peak": fma / ms * 1e3 / FMA_PEAK[dtname],
           "vjp_ms": ms_adj, "vjp_items_per_s": batch / ms_adj * 1e3, "domain_errors": errors}
    del x, y, g, d, b_t, x_t, y_t, g_t, d_t, spec, vjp, make
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--theta", type=float, default=1.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_glog.py measures on the GPU: no device visible")
    ga.init_device()
    stream = torch.cuda.current_stream()
    ga._lib.check(ga.lib().gaast_hip_set_stream(ctypes.c_void_p(stream.cuda_stream)))
    out = []
    for name, metric, grades, N in CASES:
        for dtname in ("f32", "f64"):
            out.append(case(name, metric, grades, N, dtname, args.batch, args.theta, stream, args.steps, args.warmup))
    print(json.dumps({"bench": "glog", "device": torch.cuda.get_device_name(0), "cases": out}))


if __name__ == "__main__":
    main()
