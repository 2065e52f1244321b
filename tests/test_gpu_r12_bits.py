"""The bits of k_gp_mfma32p<false, 12> are pinned: result rows recorded from the kernel as it stood before its step loop was
rewritten around lane-constant XOR deltas (tests/golden/r12_bits.npz, written by tools/record_r12_bits.py on that commit)
must come out again, np.array_equal.  Each result component is one fused multiply-add chain over a_hi ascending with the
term order mfma16_k; a change of the address arithmetic, the staging or the store phase must not move a single bit.

Inputs are numpy-seeded (helpers.rows_of), only the expected rows are stored:
  plain    R^12, full x full, 3 items (the 16-byte-piece fast path, one item per workgroup: three workgroups)
  mixed    -1 among the lo and the hi vectors (neg_lo: lane constants of the A side; neg_hi: the block signs), 1 item
  partial  a left operand without its top grades: the general staging path in front of the same step loop, 1 item
"""
import os

import numpy as np
import pytest

import gaast_amd as ga
from helpers import full_grades, hip_eval_batch, rows_of

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "r12_bits.npz")
KERNEL = "k_gp_mfma32p<false,12>"

#        name       metric                                                                      left grades            items seed
CASES = [("plain", [1.0] * 12, None, 3, 1201),
         ("mixed", [1.0, -1.0, 1.0, -1.0, 1.0, 1.0, 1.0, -1.0, 1.0, 1.0, -1.0, 1.0], None, 1, 1202),
         ("partial", [1.0] * 12, [0, 1, 2, 3, 4, 5, 6, 7, 8], 1, 1203)]


def evaluate(name):
    """the case's result rows (f32) through the library that is loaded, and the launch labels"""
    _, metric, left_grades, batch, seed = next(c for c in CASES if c[0] == name)
    n = 12
    lg = full_grades(n) if left_grades is None else left_grades

    def build(B):
        return B.input(0, lg, n) * B.input(1, full_grades(n), n)
    rng = np.random.default_rng(seed)
    rows = {0: rows_of(n, lg, batch, rng, np.float32), 1: rows_of(n, full_grades(n), batch, rng, np.float32)}
    alg = metric if any(m != 1.0 for m in metric) else n
    got, _, spec = hip_eval_batch(build, alg, rows, batch, dtype=ga.F32)
    return got, spec.launches()


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_r12_f32_rows_keep_their_recorded_bits(name):
    got, launches = evaluate(name)
    assert any(l.startswith("product_dense_mfma[") and l.split(" :: ")[-1].startswith(KERNEL) for l in launches), launches
    want = np.load(GOLDEN)[name]
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    assert np.abs(want).max() > 1.0     # a real product, not zeros
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
