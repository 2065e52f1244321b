#!/usr/bin/env python3
"""Record tests/golden/r12_bits.npz: the rows tests/test_gpu_r12_bits.py pins, from the library that is loaded.

Run it (on a GPU) on the commit whose bits are to be kept -- BEFORE a change to k_gp_mfma32p, never after: a fixture
recorded from the code under test pins nothing.  GAAST_HIP_LIB selects another build of the library.

    python3 tools/record_r12_bits.py [output.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import gaast_amd as ga                      # noqa: E402
import test_gpu_r12_bits as t               # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN
    ga.init_device(0)
    rows = {}
    for name, *_ in t.CASES:
        got, launches = t.evaluate(name)
        assert any(l.split(" :: ")[-1].startswith(t.KERNEL) for l in launches), launches
        assert got.dtype == np.float32
        rows[name] = got
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, **rows)
    print(ga.lib().gaast_hip_version().decode(), {k: v.shape for k, v in rows.items()}, "->", out)


if __name__ == "__main__":
    main()
