"""Second order through the general exponential on the MI355X: the forward (k_mv_gexp), the first-order adjoint (k_mv_gexp_adj), the
tangent (k_mv_gexp_jvp) and the second-order adjoint (k_mv_gexp_adj2) of gexp(A) in one run, f32 and f64, over the cases of
tools/bench_gexp.py.  Prints one JSON line.

Timing as bench.py: inputs resident in HBM, a warm-up, then HIP events on the launch stream around every evaluation.  Operands are
U(-1, 1) normalised to sum |A| = theta (default 3: s = 3 squarings per item).  Every program is the whole evaluation a caller pays
for: the tangent and the second-order adjoint include the copies of h (and g) into their cache buffers.  Reported per case: the four
times, their ratios to the first-order adjoint of the same run (there is no other baseline: the new steps did not exist before), and
the ratio the multiply-add counts predict (in units of N^2 per item: forward m + s, adjoint and tangent 3 (m + s), second-order
adjoint 8 m + 9 s; m = 8 / 14 Horner steps).
    python tools/bench_gexp2.py [--steps 20] [--warmup 3] [--batch 1048576] [--theta 3]
"""
import argparse
import ctypes
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402  (before gaast_amd: see tests/conftest.py)

import gaast_amd as ga  # noqa: E402
from bench_gexp import CASES, timed  # noqa: E402


def case(name, metric, grades, N, dtname, batch, theta, stream, steps, warmup):
    dtype = ga.F32 if dtname == "f32" else ga.F64
    tdt = torch.float32 if dtype == ga.F32 else torch.float64
    n = len(metric)
    spec = ga.mv(ga.Input(0, grades, n)).gexp().specialize(ga.MetricAlgebra(metric), dtype=dtype, flags=ga.FLAG_GEXP_GRAD2)
    mask, out_len = spec.output_info()
    in_len = sum(int(ga.n_choose_k(n, k)) for k in grades)
    gen = torch.Generator(device="cuda:0").manual_seed(20261021)
    new = lambda cols: torch.empty((batch, cols), device="cuda:0", dtype=tdt).uniform_(-1, 1, generator=gen)
    x_t, g_t, h_t = new(in_len), new(out_len), new(in_len)
    x_t *= theta / x_t.abs().sum(dim=1, keepdim=True)
    y_t, d_t = torch.empty_like(g_t), torch.empty_like(x_t)
    x, h, d = (ga.DeviceMV.wrap_tensor(t, n, grades) for t in (x_t, h_t, d_t))
    g, y = (ga.DeviceMV.wrap_tensor(t, n, ga.GradeSet(mask)) for t in (g_t, y_t))
    vjp, jvp = spec.vjp(0), spec.jvp(0)
    adj2 = vjp.vjp(0)
    ms = {"forward": timed(lambda: spec.eval_batch([x], batch, out=y), stream, steps, warmup),
          "adjoint": timed(lambda: vjp.eval_batch([x], g, batch, out=d), stream, steps, warmup),
          "jvp": timed(lambda: jvp.eval_batch([x], h, batch, out=y), stream, steps, warmup),
          "adjoint2": timed(lambda: adj2.eval_batch([x, g], h, batch, out=d), stream, steps, warmup)}
    m = 8 if dtype == ga.F32 else 14
    s = max(0, math.ceil(math.log2(theta)) + 1) if theta > 0.5 else 0
    fma = {"forward": m + s, "adjoint": 3 * (m + s), "jvp": 3 * (m + s), "adjoint2": 8 * m + 9 * s}
    res = {"case": name, "N": N, "dtype": dtname, "batch": batch, "theta": theta, "squarings": s, "ms": ms,
           "ratio_to_adjoint": {k: v / ms["adjoint"] for k, v in ms.items()},
           "predicted_ratio_to_adjoint": {k: v / fma["adjoint"] for k, v in fma.items()},
           "TFMA_s": {k: float(batch) * fma[k] * N * N / ms[k] / 1e9 for k in ms},
           "launches": {"jvp": jvp.launches(), "adjoint2": adj2.launches()}, "domain_errors": spec.domain_errors()}
    del x, y, g, h, d, x_t, y_t, g_t, h_t, d_t, spec, vjp, jvp, adj2
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
        raise SystemExit("bench_gexp2.py measures on the GPU: no device visible")
    ga.init_device()
    stream = torch.cuda.current_stream()
    ga._lib.check(ga.lib().gaast_hip_set_stream(ctypes.c_void_p(stream.cuda_stream)))
    out = []
    for name, metric, grades, N in CASES:
        for dtname in ("f32", "f64"):
            out.append(case(name, metric, grades, N, dtname, args.batch, args.theta, stream, args.steps, args.warmup))
    print(json.dumps({"bench": "gexp2", "device": torch.cuda.get_device_name(0), "cases": out}))


if __name__ == "__main__":
    main()
