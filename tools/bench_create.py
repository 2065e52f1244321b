"""What gaast_hip_program_create costs, with and without the kernel cache (include/gaast_hip.h: gaast_hip_jit_cache_*).

For the programs of bench.py's workloads cl41, cl41s, vinv8, proj12, sand9g1 and cfg1_8, and for the three programs behind the
torch_fn of a PGA3D motor sandwich (the forward and one VJP per input), the time of the gaast_hip_program_create call alone:

    cold              a fresh process, an empty cache directory                (compiles, stores)
    warm from disk    a fresh process, the directory a cold process has filled (reads, checks, hipModuleLoadData)
    warm in memory    the same program created again in that process, the first still alive (shares the loaded modules)

One fresh process per program and case, --procs of them; the table gives the median and the range [min .. max] over the
processes, in milliseconds.  Warm in memory is taken from the second creation of the warm-from-disk processes.  A library
without the cache (a checkout before it) has only the cold case; its second creation in the process is listed as "again".

    python tools/bench_create.py [--procs 7]
"""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gaast_amd as ga  # noqa: E402
from gaast_amd import _lib  # noqa: E402

WORKLOADS = ("cl41", "cl41s", "vinv8", "proj12", "sand9g1", "cfg1_8")
UNITS = WORKLOADS + ("pga3d_torch_fn",)
HAS_CACHE = hasattr(ga, "jit_cache_dir")
CHILD_TIMEOUT_S = 300


def programs_of(unit):
    """[(label, ProgramDesc, objects that own its memory)]"""
    if unit == "pga3d_torch_fn":
        n, metric = 4, [0.0, 1.0, 1.0, 1.0]
        M, X = ga.mv(ga.Input(0, [0, 2, 4], n)), ga.mv(ga.Input(1, [3], n))
        spec = (M * X * M.rev()).specialize(metric, dtype=ga.F32)
        vjps = [spec.vjp(0), spec.vjp(1)]
        return [("forward", spec.program_desc(), spec), ("vjp motor", vjps[0].desc, vjps[0]), ("vjp point", vjps[1].desc, vjps[1])]
    import bench
    wl = bench.workload_spec(unit)
    exprs = [ga.mv(ga.Input(s, g, wl["n"])) for s, g in enumerate(wl["inputs"])]
    spec = wl["build"](*exprs).specialize(ga.MetricAlgebra(wl["metric"]), dtype=wl["dtype"], flags=wl.get("flags", 0))
    return [(unit, spec.program_desc(), spec)]


def create_ms(desc):
    L = _lib.lib()
    h = C.c_void_p()
    t0 = time.perf_counter()
    st = L.gaast_hip_program_create(C.byref(desc), C.byref(h))
    dt = (time.perf_counter() - t0) * 1e3
    _lib.check(st)
    return dt, h


def child(unit, cache_dir):
    ga.init_device(0)
    if cache_dir:
        ga.jit_cache_dir(cache_dir)
    progs = programs_of(unit)
    L = _lib.lib()
    first, second, handles = [], [], []
    for _, desc, _ in progs:
        dt, h = create_ms(desc)
        first.append(dt)
        handles.append(h)
    launches = [[L.gaast_hip_program_launch_name(h, i).decode() for i in range(L.gaast_hip_program_num_launches(h))] for h in handles]
    for _, desc, _ in progs:
        dt, h = create_ms(desc)
        second.append(dt)
        handles.append(h)
    stats = ga.jit_cache_stats() if HAS_CACHE else None
    for h in handles:
        L.gaast_hip_program_destroy(h)
    print(json.dumps(dict(unit=unit, labels=[p[0] for p in progs], first_ms=first, second_ms=second, stats=stats, launches=launches)))


def run_child(unit, cache_dir):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", unit, "--dir", cache_dir or ""],
                       capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    if r.returncode != 0:
        # nothing more is started on the GPU after a process that failed
        raise SystemExit(f"{unit}: child ended with status {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-4000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def summary(values):
    return f"{statistics.median(values):9.2f} [{min(values):8.2f} .. {max(values):8.2f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=7, help="fresh processes per program and case")
    ap.add_argument("--child", default=None)
    ap.add_argument("--dir", default="")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.dir)

    print(f"# {_lib.lib().gaast_hip_version().decode()}; kernel cache: {'yes' if HAS_CACHE else 'no'}; {args.procs} fresh processes per case")
    rows = []   # (program label, {case: [ms per process]}, note)
    for unit in UNITS:
        cases = {"cold": [], "again": []}
        note = ""
        base = tempfile.mkdtemp(prefix="gaast_bench_create_")
        try:
            for p in range(args.procs):
                d = os.path.join(base, f"cold{p}") if HAS_CACHE else None
                r = run_child(unit, d)
                print("cold", json.dumps(r))
                cases["cold"].append(r["first_ms"])
                cases["again"].append(r["second_ms"])
            if HAS_CACHE:
                cases["disk"], cases["memory"] = [], []
                filled = os.path.join(base, "cold0")
                files = [os.path.getsize(os.path.join(filled, f)) for f in sorted(os.listdir(filled))]
                note = f"{len(files)} code objects, {sum(files)} bytes"
                for p in range(args.procs):
                    r = run_child(unit, filled)
                    print("warm", json.dumps(r))
                    assert r["stats"]["compiled"] == 0, r["stats"]
                    cases["disk"].append(r["first_ms"])
                    cases["memory"].append(r["second_ms"])
        finally:
            shutil.rmtree(base, ignore_errors=True)
        labels = r["labels"]
        for i, label in enumerate(labels):
            rows.append((label if len(labels) == 1 else f"{unit}: {label}", {c: [v[i] for v in vs] for c, vs in cases.items()}, note if i == 0 else ""))
        if len(labels) > 1:
            rows.append((f"{unit}: all {len(labels)}", {c: [sum(v) for v in vs] for c, vs in cases.items()}, ""))

    cols = ["cold", "disk", "memory"] if HAS_CACHE else ["cold", "again"]
    heads = {"cold": "cold", "disk": "warm from disk", "memory": "warm in memory", "again": "again, same process"}
    print()
    print(f"# gaast_hip_program_create, ms: median [min .. max] over {args.procs} fresh processes")
    print(f"{'program':28s} " + " ".join(f"{heads[c]:>31s}" for c in cols))
    for label, cases, note in rows:
        print(f"{label:28s} " + " ".join(summary(cases[c]) for c in cols) + (f"   ({note})" if note else ""))


if __name__ == "__main__":
    main()
