"""Forward mode through the general square root and logarithm on the MI355X: for gsqrt and for glog the forward, the first-order
adjoint (k_mv_gsqrt_adj / k_mv_glog_adj) and the tangent (k_mv_gsqrt_jvp / k_mv_jvp_glog), and the composed second-order gradient of
gsqrt (vjp(0).vjp(0): two adjoint solves, one tangent solve and two adjoint products), all in one run, f32 and f64, over the cases of
tools/bench_glog.py.  Prints one JSON line.

Timing as bench.py: inputs resident in HBM, a warm-up, then HIP events on the launch stream around every evaluation.  Operands are
A = gexp(B), B = U(-1, 1) normalised to sum |B| = theta (default 1: two or three roots of the logarithm).  Every program is the whole
evaluation a caller pays for: the tangents include the copy of h into its cache buffer.  Reported per case: the times and their
ratios to the first-order adjoint of the same function in the same run -- there is no other baseline, the new steps did not exist
before.  Prediction: a tangent runs the eliminations of its adjoint (root steps + 1 for gsqrt, the roots' steps + s + 14 for glog),
so its ratio is 1.0; the composed second-order gradient recomputes the root in four nodes and adds two products.
    python tools/bench_root_log_jvp.py [--steps 20] [--warmup 3] [--batch 1048576] [--theta 1]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402  (before gaast_amd: see tests/conftest.py)

import gaast_amd as ga  # noqa: E402
from bench_glog import CASES, timed  # noqa: E402


def case(name, metric, grades, N, dtname, batch, theta, stream, steps, warmup):
    dtype = ga.F32 if dtname == "f32" else ga.F64
    tdt = torch.float32 if dtype == ga.F32 else torch.float64
    n = len(metric)
    alg = ga.MetricAlgebra(metric)
    make = ga.mv(ga.Input(0, grades, n)).gexp().specialize(alg, dtype=dtype)
    mask, row_len = make.output_info()
    sgrades = [k for k in range(n + 1) if (mask >> k) & 1]        # the grades of the blade set: operand, tangent and result
    in_len = sum(int(ga.n_choose_k(n, k)) for k in grades)
    gen = torch.Generator(device="cuda:0").manual_seed(20261021)
    b_t = torch.empty((batch, in_len), device="cuda:0", dtype=tdt).uniform_(-1, 1, generator=gen)
    b_t *= theta / b_t.abs().sum(dim=1, keepdim=True)
    new = lambda: torch.empty((batch, row_len), device="cuda:0", dtype=tdt)
    x_t, y_t, d_t = new(), new(), new()
    g_t, h_t = new().uniform_(-1, 1, generator=gen), new().uniform_(-1, 1, generator=gen)
    sset = ga.GradeSet(mask)
    x, y, d, g, h = (ga.DeviceMV.wrap_tensor(t, n, sset) for t in (x_t, y_t, d_t, g_t, h_t))
    make.eval_batch([ga.DeviceMV.wrap_tensor(b_t, n, grades)], batch, out=x)      # A = gexp(B)
    torch.cuda.synchronize()
    res = {"case": name, "N": N, "dtype": dtname, "batch": batch, "theta": theta}
    for fn in ("gsqrt", "glog"):
        e = ga.mv(ga.Input(0, sgrades, n))
        spec = (e.gsqrt() if fn == "gsqrt" else e.glog()).specialize(alg, dtype=dtype, flags=ga.FLAG_GSQRT_GLOG_JVP)
        vjp, jvp = spec.vjp(0), spec.jvp(0)
        ms = {"forward": timed(lambda: spec.eval_batch([x], batch, out=y), stream, steps, warmup),
              "adjoint": timed(lambda: vjp.eval_batch([x], g, batch, out=d), stream, steps, warmup),
              "jvp": timed(lambda: jvp.eval_batch([x], h, batch, out=y), stream, steps, warmup)}
        launches = {"jvp": jvp.launches()}
        if fn == "gsqrt":
            adj2 = vjp.vjp(0)
            ms["adjoint2"] = timed(lambda: adj2.eval_batch([x, g], h, batch, out=d), stream, steps, warmup)
            launches["adjoint2"] = adj2.launches()
        res[fn] = {"ms": ms, "ratio_to_adjoint": {k: v / ms["adjoint"] for k, v in ms.items()}, "predicted_jvp_ratio": 1.0,
                   "launches": launches, "domain_errors": spec.domain_errors()}
        del spec, vjp, jvp
    del x, y, d, g, h, b_t, x_t, y_t, d_t, g_t, h_t, make
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
        raise SystemExit("bench_root_log_jvp.py measures on the GPU: no device visible")
    ga.init_device()
    stream = torch.cuda.current_stream()
    ga._lib.check(ga.lib().gaast_hip_set_stream(ctypes.c_void_p(stream.cuda_stream)))
    out = []
    for name, metric, grades, N in CASES:
        for dtname in ("f32", "f64"):
            out.append(case(name, metric, grades, N, dtname, args.batch, args.theta, stream, args.steps, args.warmup))
    print(json.dumps({"bench": "root_log_jvp", "device": torch.cuda.get_device_name(0), "cases": out}))


if __name__ == "__main__":
    main()
