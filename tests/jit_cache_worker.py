"""One fresh process of tests/test_gpu_jit_cache.py (the kernel cache is a property of a process and of a directory):

    python jit_cache_worker.py run <cache dir | ->               every program once; prints launches, result rows, counters
    python jit_cache_worker.py share                             two SpecializedAst of one expression share their modules
    python jit_cache_worker.py jitfails <cache dir | ->          GAAST_FLAG_DEBUG_JIT_FAILS, cold and against warm caches

The last line printed is one JSON object.
"""
import gc
import json
import os
import sys

import numpy as np
import torch  # noqa: F401  (before gaast_amd: tests/conftest.py says why)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gaast_amd as ga  # noqa: E402

R41 = [1.0, 1.0, 1.0, 1.0, -1.0]
R63 = [1.0] * 6 + [-1.0] * 3


def _even(n):
    return [k for k in range(n + 1) if k % 2 == 0]


def _full(n):
    return list(range(n + 1))


# name -> (metric, grades of the inputs, slots shared by all items, expression, flags): bench.py's workloads of these names
PROGRAMS = {
    "cl41s": (R41, [[0, 2, 4], [1]], [0], lambda r, x: r * x * r.rev(), 0),                       # two builds: exact + contracted
    "vinv8": ([1.0] * 8, [_even(8)], [], lambda a: a.vinv(), 0),                                  # slabs in LDS
    "proj12": ([1.0] * 12, [[1], [2]], [], lambda v, bv: (v & bv) & bv.vinv(), 0),                # register trial
    "sand9g1": (R63, [_even(9), [1]], [], lambda r, x: (r * x * r.rev()).g(1), 0),                # gaast_chain
    "sand9g1x": (R63, [_even(9), [1]], [], lambda r, x: (r * x * r.rev()).g(1), ga.FLAG_EXACT_ORDER),
    "cfg1_8": ([1.0] * 8, [_full(8)] * 3, [], lambda a, b, c: (a + b * c).g(2), 0),               # single long-row list
    "cfg1_8x": ([1.0] * 8, [_full(8)] * 3, [], lambda a, b, c: (a + b * c).g(2), ga.FLAG_EXACT_ORDER),
}
BATCH = 193


def make(name, extra_flags=0):
    metric, grades, _, build, flags = PROGRAMS[name]
    n = len(metric)
    exprs = [ga.mv(ga.Input(s, g, n)) for s, g in enumerate(grades)]
    return build(*exprs).specialize(ga.MetricAlgebra(metric), flags=flags | extra_flags)


def rows_for(name):
    metric, grades, shared, _, _ = PROGRAMS[name]
    n = len(metric)
    rng = np.random.default_rng(sorted(PROGRAMS).index(name))
    return [rng.uniform(-1.0, 1.0, (1 if s in shared else BATCH, ga.graded.row_len(n, ga.graded._mask_of(g)))) for s, g in enumerate(grades)]


def evaluate(spec, name):
    out = spec.eval_batch(rows_for(name), BATCH)
    ga.lib().gaast_hip_synchronize()
    return np.ascontiguousarray(out.download_rows()).tobytes().hex()


def files_under(path):
    return sorted(os.path.join(d, f)[len(path):] for d, _, fs in os.walk(path) for f in fs)


def cmd_run(cache_dir):
    before = files_under(os.getcwd())
    if cache_dir != "-":
        ga.jit_cache_dir(cache_dir)
    launches, rows, per_program, keep = {}, {}, {}, []
    for name in PROGRAMS:
        s0 = ga.jit_cache_stats()
        spec = make(name)
        keep.append(spec)   # alive to the end: a kernel two programs have in common is then one compilation and one file
        launches[name] = spec.launches()
        rows[name] = evaluate(spec, name)
        s1 = ga.jit_cache_stats()
        per_program[name] = {k: s1[k] - s0[k] for k in s1}
    return dict(launches=launches, rows=rows, stats=ga.jit_cache_stats(), per_program=per_program,
                new_files_in_cwd=[f for f in files_under(os.getcwd()) if f not in before])


def cmd_share():
    report = {}
    for name in ("cl41s", "sand9g1x", "vinv8"):
        base = ga.jit_cache_stats()
        first = make(name)
        want = evaluate(first, name)
        s1 = ga.jit_cache_stats()
        second = make(name)
        labels = second.launches()
        s2 = ga.jit_cache_stats()
        assert s1["compiled"] > base["compiled"], (name, base, s1)
        assert s2["compiled"] == s1["compiled"] and s2["memory_hits"] > s1["memory_hits"], (name, s1, s2)
        assert s2["live_modules"] == s1["live_modules"] > base["live_modules"], (name, base, s1, s2)
        assert labels == first.launches(), (labels, first.launches())
        assert evaluate(second, name) == want
        del first
        gc.collect()
        s3 = ga.jit_cache_stats()
        assert s3["live_modules"] == s2["live_modules"], (name, s2, s3)      # the second program keeps every module loaded
        assert evaluate(second, name) == want, name                          # ... and they still run, to the same bits
        del second
        gc.collect()
        s4 = ga.jit_cache_stats()
        assert s4["live_modules"] == base["live_modules"], (name, base, s4)  # unloaded with the last holder, not at exit
        # nothing is kept alive by the map: the next program compiles again
        third = make(name)
        assert evaluate(third, name) == want
        s5 = ga.jit_cache_stats()
        assert s5["compiled"] > s4["compiled"] and s5["memory_hits"] == s4["memory_hits"], (name, s4, s5)
        del third
        gc.collect()
        report[name] = dict(modules=s1["live_modules"] - base["live_modules"], labels=labels)
    assert ga.jit_cache_stats()["live_modules"] == 0
    return report


def cmd_jitfails(cache_dir):
    """labels and rows of every program under GAAST_FLAG_DEBUG_JIT_FAILS; with a directory: after the same programs have been
    created without the flag (and are still alive), so that both cache levels hold every kernel the flag must not find"""
    keep = []
    if cache_dir != "-":
        ga.jit_cache_dir(cache_dir)
        for name in PROGRAMS:
            keep.append(make(name))
            keep[-1].program()
    warm = ga.jit_cache_stats()
    launches, rows = {}, {}
    for name in PROGRAMS:
        spec = make(name, ga.FLAG_DEBUG_JIT_FAILS)
        launches[name] = spec.launches()
        rows[name] = evaluate(spec, name)
    return dict(launches=launches, rows=rows, warm=warm, stats=ga.jit_cache_stats())


if __name__ == "__main__":
    mode = sys.argv[1]
    result = cmd_run(sys.argv[2]) if mode == "run" else cmd_share() if mode == "share" else cmd_jitfails(sys.argv[2])
    print(json.dumps(result))
