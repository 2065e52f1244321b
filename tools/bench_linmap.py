"""Outermorphisms on the MI355X: gaast_hip_linmap_apply at n = 5 and n = 12 (f32 and f64), and the R^12 f32 full geometric product
in a random non-diagonal Gram algebra against the same product in OrthoEuclidN(12).  Prints one JSON line.

Timing as bench.py: inputs resident in HBM, a warm-up, then HIP events on the launch stream around every launch.
    python tools/bench_linmap.py [--steps 20] [--warmup 3]
    python tools/bench_linmap.py --vjp      the adjoints instead: apply_transposed against apply (alternating, same rows), and
                                            matrix_vjp at n = 4, 5, 6, 8 as a fraction of 8 TB/s of its algorithmic bytes (the two rows)
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

HBM_BPS = 8.0e12
PEAK = {"f32": 157.3e12, "f64": 78.6e12}


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


def linmap_case(n, batch, dtname, stream, steps, warmup):
    dtype = ga.F32 if dtname == "f32" else ga.F64
    tdt = torch.float32 if dtype == ga.F32 else torch.float64
    rng = np.random.default_rng(n)
    q = np.linalg.qr(rng.uniform(-1, 1, (n, n)))[0]
    f = ga.Outermorphism(q, dtype)
    full = list(range(n + 1))
    x_t = torch.empty((batch, 1 << n), device="cuda:0", dtype=tdt).uniform_(-1, 1)
    y_t = torch.empty_like(x_t)
    x, y = ga.DeviceMV.wrap_tensor(x_t, n, full), ga.DeviceMV.wrap_tensor(y_t, n, full)
    ms = timed(lambda: f.apply(x, y), stream, steps, warmup)
    macs = sum(int(ga.n_choose_k(n, k)) ** 2 for k in range(n + 1))
    flops, bytes_ = 2.0 * macs * batch, 2.0 * batch * (1 << n) * x_t.element_size()
    res = {"n": n, "dtype": dtname, "batch": batch, "ms": ms, "GB_s": bytes_ / ms / 1e6, "TFLOP_s": flops / ms / 1e9,
           "frac_hbm_8TBs": bytes_ / ms / 1e-3 / HBM_BPS, "frac_peak": flops / ms / 1e-3 / PEAK[dtname]}
    del x, y, x_t, y_t, f
    torch.cuda.empty_cache()
    return res


def transposed_case(n, batch, dtname, stream, steps, warmup):
    """apply and apply_transposed of one map on the same rows, alternating so that both see the same clocks"""
    dtype = ga.F32 if dtname == "f32" else ga.F64
    tdt = torch.float32 if dtype == ga.F32 else torch.float64
    f = ga.Outermorphism(np.linalg.qr(np.random.default_rng(n).uniform(-1, 1, (n, n)))[0], dtype)
    full = list(range(n + 1))
    x_t = torch.empty((batch, 1 << n), device="cuda:0", dtype=tdt).uniform_(-1, 1)
    y_t = torch.empty_like(x_t)
    x, y = ga.DeviceMV.wrap_tensor(x_t, n, full), ga.DeviceMV.wrap_tensor(y_t, n, full)
    ms = {"apply": [], "apply_transposed": []}
    for _ in range(3):
        ms["apply"].append(timed(lambda: f.apply(x, y), stream, steps, warmup))
        ms["apply_transposed"].append(timed(lambda: f.apply_transposed(x, y), stream, steps, warmup))
    res = {"n": n, "dtype": dtname, "batch": batch, "ms_apply": ms["apply"], "ms_apply_transposed": ms["apply_transposed"],
           "transposed_over_apply": min(ms["apply_transposed"]) / min(ms["apply"])}
    del x, y, x_t, y_t, f
    torch.cuda.empty_cache()
    return res


def matrix_vjp_case(n, batch, dtname, stream, steps, warmup):
    dtype = ga.F32 if dtname == "f32" else ga.F64
    tdt = torch.float32 if dtype == ga.F32 else torch.float64
    f = ga.Outermorphism(np.random.default_rng(n).uniform(-1, 1, (n, n)), dtype)
    full = list(range(n + 1))
    x_t = torch.empty((batch, 1 << n), device="cuda:0", dtype=tdt).uniform_(-1, 1)
    g_t = torch.empty_like(x_t).uniform_(-1, 1)
    dm = torch.empty((n, n), device="cuda:0", dtype=tdt)
    x, g = ga.DeviceMV.wrap_tensor(x_t, n, full), ga.DeviceMV.wrap_tensor(g_t, n, full)
    ms = timed(lambda: f.matrix_vjp(x, g, out=dm), stream, steps, warmup)
    bytes_ = 2.0 * batch * (1 << n) * x_t.element_size()
    res = {"n": n, "dtype": dtname, "batch": batch, "ms": ms, "GB_s": bytes_ / ms / 1e6, "frac_hbm_8TBs": bytes_ / ms / 1e-3 / HBM_BPS}
    del x, g, x_t, g_t, f
    torch.cuda.empty_cache()
    return res


def gram_product_case(stream, steps, warmup, batch=65536):
    n = 12
    rng = np.random.default_rng(12)
    a = rng.uniform(-1, 1, (n, n))
    g = (a + a.T) / 2
    full = list(range(n + 1))
    out = {}
    for name, alg in (("gram", ga.GramAlgebra(g)), ("ortho", ga.OrthoEuclidN(n))):
        spec = (ga.mv(ga.Input(0, full, n)) * ga.mv(ga.Input(1, full, n))).specialize(alg, dtype=ga.F32)
        ins_t = [torch.empty((batch, 1 << n), device="cuda:0", dtype=torch.float32).uniform_(-1, 1) for _ in range(2)]
        ins = [ga.DeviceMV.wrap_tensor(t, n, full) for t in ins_t]
        o_t = torch.empty((batch, 1 << n), device="cuda:0", dtype=torch.float32)
        o = ga.DeviceMV.wrap_tensor(o_t, n, full)
        ms = timed(lambda: spec.eval_batch(ins, batch, out=o), stream, steps, warmup)
        out[name] = {"ms": ms, "launches": spec.launches()}
        del spec, ins, ins_t, o, o_t
        torch.cuda.empty_cache()
    out["batch"] = batch
    out["gram_over_ortho"] = out["gram"]["ms"] / out["ortho"]["ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vjp", action="store_true", help="time the adjoints (apply_transposed, matrix_vjp) instead")
    args = ap.parse_args()
    ga.init_device(0)
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    ga._lib.check(ga.lib().gaast_hip_set_stream(ctypes.c_void_p(stream.cuda_stream)))
    if args.vjp:
        res = {"tool": "bench_linmap --vjp", "version": ga.lib().gaast_hip_version().decode(), "apply_transposed": [], "matrix_vjp": []}
        for n, batch in ((5, 1 << 22), (12, 65536)):
            for dt in ("f32", "f64"):
                res["apply_transposed"].append(transposed_case(n, batch, dt, stream, args.steps, args.warmup))
        for n, batch in ((4, 1 << 22), (5, 1 << 22), (6, 1 << 22), (8, 1 << 18)):
            for dt in ("f32", "f64"):
                res["matrix_vjp"].append(matrix_vjp_case(n, batch, dt, stream, args.steps, args.warmup))
        print(json.dumps(res))
        return
    res = {"tool": "bench_linmap", "version": ga.lib().gaast_hip_version().decode(), "linmap": []}
    for n, batch in ((5, 1 << 22), (12, 65536)):
        for dt in ("f32", "f64"):
            res["linmap"].append(linmap_case(n, batch, dt, stream, args.steps, args.warmup))
    res["r12_f32_gp"] = gram_product_case(stream, args.steps, args.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
