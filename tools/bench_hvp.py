"""Second-order reverse mode and forward mode on the MI355X: for three workloads, the time of the forward program, of one first-order
VJP, of the second-order program with respect to the other operand (the inner step of a Hessian-vector product) and of the JVP
(SpecializedAst.jvp), all in one run.  Prints one JSON line.

Timing as bench.py: inputs resident in HBM, a warm-up, then HIP events on the launch stream around every evaluation.  Per case:
milliseconds per evaluation, the ratio to the forward of the same run, and the launch names of each program.
    python tools/bench_hvp.py [--steps 20] [--warmup 3] [--scale 1.0]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before gaast_amd: see tests/conftest.py)

import gaast_amd as ga  # noqa: E402


def _inp(slot, grades, n):
    return ga.mv(ga.Input(slot, grades, n))


def _product(n):
    full = list(range(n + 1))
    return _inp(0, full, n) * _inp(1, full, n)


def _sandwich():
    M, X = _inp(0, [0, 2, 4], 4), _inp(1, [3], 4)
    return M * X * M.rev()


CASES = [   # name, expression, metric, dtype, batch
    ("R12 product f32", lambda: _product(12), [1.0] * 12, "f32", 1 << 14),
    ("R6 product f32", lambda: _product(6), [1.0] * 6, "f32", 1 << 20),
    ("PGA3D sandwich f64", _sandwich, [0.0, 1.0, 1.0, 1.0], "f64", 1 << 20),
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


def case(name, build, metric, dtname, batch, stream, steps, warmup):
    dtype = ga.F32 if dtname == "f32" else ga.F64
    tdt = torch.float32 if dtype == ga.F32 else torch.float64
    n = len(metric)
    spec = build().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    d = spec.program_desc()
    lay = [(d.inputs[s].storage_dim, d.inputs[s].grade_mask) for s in range(2)]
    out_mask, out_len = spec.output_info()
    lay.append((n, out_mask))                      # slots 0, 1 and the cotangent
    gen = torch.Generator(device="cuda:0").manual_seed(20261021)

    def rows(dim, mask):
        t = torch.empty((batch, ga.graded.row_len(dim, mask)), device="cuda:0", dtype=tdt).uniform_(-1, 1, generator=gen)
        return t, ga.DeviceMV.wrap_tensor(t, dim, ga.GradeSet(mask))
    keep = [rows(*l) for l in lay]                 # a, b, g
    a, b, g = (mv for _, mv in keep)
    outs = [rows(*l) for l in lay]                 # result rows in the layout of a, b and the root
    oa, ob, oy = (mv for _, mv in outs)
    ha = rows(*lay[0])                             # a second cotangent / a tangent, in the layout of a
    v = spec.vjp(0)                                # d/da
    w = v.vjp(1)                                   # d/db of <h, d/da>: the other operand
    j = spec.jvp(0)
    progs = {
        "forward": (spec, lambda: spec.eval_batch([a, b], batch, out=oy)),
        "vjp": (v, lambda: v.eval_batch([a, b], g, batch, out=oa)),
        "vjp2": (w, lambda: w.eval_batch([a, b, g], ha[1], batch, out=ob)),
        "jvp": (j, lambda: j.eval_batch([a, b], ha[1], batch, out=oy)),
    }
    res = {"case": name, "dtype": dtname, "batch": batch}
    for key, (prog, fn) in progs.items():
        res[key + "_ms"] = timed(fn, stream, steps, warmup)
        res[key + "_launches"] = prog.launches()
    for key in ("vjp", "vjp2", "jvp"):
        res[key + "_over_forward"] = res[key + "_ms"] / res["forward_ms"]
    del keep, outs, ha, a, b, g, oa, ob, oy, progs, spec, v, w, j
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every case's batch")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hvp.py measures on the GPU: no device visible")
    ga.init_device()
    stream = torch.cuda.current_stream()
    ga._lib.check(ga.lib().gaast_hip_set_stream(ctypes.c_void_p(stream.cuda_stream)))
    out = [case(name, build, metric, dtname, max(1, int(batch * args.scale)), stream, args.steps, args.warmup)
           for name, build, metric, dtname, batch in CASES]
    print(json.dumps({"bench": "hvp", "device": torch.cuda.get_device_name(0), "version": ga.lib().gaast_hip_version().decode(), "cases": out}))


if __name__ == "__main__":
    main()
