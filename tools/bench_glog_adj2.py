"""Second order through the general logarithm on the MI355X: the forward (k_mv_glog), the first-order adjoint (k_mv_glog_adj) and the
second-order adjoint node (vjp(0).vjp(0): one k_mv_adj2_glog launch and the copies of g and h into their cache buffers), all in one
run, f32 and f64, over R3, PGA3D-even, PGA3D, CGA and R33 of tools/bench_glog.py.  Prints one JSON line.

Timing as bench.py: inputs resident in HBM, a warm-up, then HIP events on the launch stream around every evaluation.  Operands are
A = gexp(B), B = U(-1, 1) normalised to sum |B| = theta (default 1: two or three roots of the logarithm).  Reported per case: the times
and the ratio of the new node to the first-order adjoint of the same run -- there is no other baseline, the step did not exist
before.  Prediction from elimination counts: the adjoint runs k + s + 14 (k root steps, s roots), the new node k + 3 s + 35, so the
ratio is (k + 3 s + 35) / (k + s + 14) with the k and s that DESIGN.md section 17 tabulates per case: about 2.
    python tools/bench_glog_adj2.py [--steps 20] [--warmup 3] [--batch 262144] [--theta 1]
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

NAMES = ("R3", "PGA3D-even", "PGA3D", "CGA", "R33")
# mean roots s and root steps k at theta = 1 (the timing table), by (case, dtype)
ROOTS_STEPS = {("R3", "f32"): (2.52, 7.5), ("R3", "f64"): (2.44, 10.3), ("PGA3D-even", "f32"): (3.00, 8.7), ("PGA3D-even", "f64"): (3.00, 12.2),
               ("PGA3D", "f32"): (2.52, 7.0), ("PGA3D", "f64"): (2.45, 9.7), ("CGA", "f32"): (2.52, 7.0), ("CGA", "f64"): (2.52, 9.9),
               ("R33", "f32"): (2.53, 6.1), ("R33", "f64"): (2.55, 9.6)}


def case(name, metric, grades, N, dtname, batch, theta, stream, steps, warmup):
    dtype = ga.F32 if dtname == "f32" else ga.F64
    tdt = torch.float32 if dtype == ga.F32 else torch.float64
    n = len(metric)
    alg = ga.MetricAlgebra(metric)
    make = ga.mv(ga.Input(0, grades, n)).gexp().specialize(alg, dtype=dtype)
    mask, row_len = make.output_info()
    sgrades = [k for k in range(n + 1) if (mask >> k) & 1]        # the grades of the blade set: operand, both cotangents and result
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
    spec = ga.mv(ga.Input(0, sgrades, n)).glog().specialize(alg, dtype=dtype, flags=ga.FLAG_GSQRT_GLOG_JVP | ga.FLAG_GLOG_GRAD2)
    vjp = spec.vjp(0)
    adj2 = vjp.vjp(0)
    ms = {"forward": timed(lambda: spec.eval_batch([x], batch, out=y), stream, steps, warmup),
          "adjoint": timed(lambda: vjp.eval_batch([x], g, batch, out=d), stream, steps, warmup),
          "adjoint2": timed(lambda: adj2.eval_batch([x, g], h, batch, out=d), stream, steps, warmup)}
    s, k = ROOTS_STEPS[(name, dtname)]
    res = {"case": name, "N": N, "dtype": dtname, "batch": batch, "theta": theta, "ms": ms, "ratio_to_adjoint": ms["adjoint2"] / ms["adjoint"],
           "predicted_ratio": (k + 3 * s + 35) / (k + s + 14) if theta == 1.0 else None, "launches": adj2.launches(), "domain_errors": spec.domain_errors()}
    del spec, vjp, adj2, x, y, d, g, h, b_t, x_t, y_t, d_t, g_t, h_t, make
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1 << 18)
    ap.add_argument("--theta", type=float, default=1.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_glog_adj2.py measures on the GPU: no device visible")
    ga.init_device()
    stream = torch.cuda.current_stream()
    ga._lib.check(ga.lib().gaast_hip_set_stream(ctypes.c_void_p(stream.cuda_stream)))
    out = []
    for name, metric, grades, N in CASES:
        if name not in NAMES:
            continue
        for dtname in ("f32", "f64"):
            out.append(case(name, metric, grades, N, dtname, args.batch, args.theta, stream, args.steps, args.warmup))
    print(json.dumps({"bench": "glog_adj2", "device": torch.cuda.get_device_name(0), "cases": out}))


if __name__ == "__main__":
    main()
