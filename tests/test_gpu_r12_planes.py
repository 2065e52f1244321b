"""k_gp_mfma32p<false, 12, *, *> on the quad-plane B image (gaast_amd/csrc/device/mfma32p_b_planes.hip.hpp): what the
pinned rows of tests/test_gpu_r12_bits.py (one item per workgroup) do not reach.

  * a persistent workgroup's SECOND and later items: the A addresses restored by the second xor of the chunk loop, the two
    live B addresses initialised again, the register prefetch of the next item's rows live.  Rows of a batch that gives
    every workgroup two items and some a third must be, bit for bit, the rows the same operands give as a batch of five
    (one item per workgroup: the path the golden file pins).
  * the chained instantiation <false, 12, false, true> (the left operand evaluated from a list while staging: general
    staging in front of the same step loop) against the f64 kernel, within the f32 bound of tests/test_gpu_dense_oracle.py
    at n = 12: 4 eps sum|terms| per component.
"""
import numpy as np
import pytest

import gaast_amd as ga
from helpers import abs_terms_bound, bits_to_row, full_grades, hip_eval_batch, row_to_bits, rows_of

pytestmark = pytest.mark.gpu


def test_later_items_of_a_workgroup_keep_the_bits_of_the_first():
    import torch
    n = 12
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    batch = 2 * cus * 2 + 3            # two workgroups per CU (64 KiB of images each): two items each, three workgroups a third
    fg = full_grades(n)

    def build(B):
        return B.input(0, fg, n) * B.input(1, fg, n)
    rng = np.random.default_rng(1212)
    rows = {0: rows_of(n, fg, batch, rng, np.float32), 1: rows_of(n, fg, batch, rng, np.float32)}
    got, _, spec = hip_eval_batch(build, n, rows, batch, dtype=ga.F32)
    assert any(l.split(" :: ")[-1].startswith("k_gp_mfma32p<false,12>") for l in spec.launches()), spec.launches()
    pick = [0, batch // 3, batch // 2, (3 * batch) // 4 + 1, batch - 1]
    five = {s: np.ascontiguousarray(r[pick]) for s, r in rows.items()}
    want, _, spec5 = hip_eval_batch(build, n, five, len(pick), dtype=ga.F32)
    assert any(l.split(" :: ")[-1].startswith("k_gp_mfma32p<false,12>") for l in spec5.launches()), spec5.launches()
    assert np.abs(want).max() > 1.0     # a real product, not zeros
    for j, i in enumerate(pick):
        differ = int((got[i].view(np.uint32) != want[j].view(np.uint32)).sum())
        print(f"row {i} of {batch}: {differ} of {got.shape[1]} words differ from the batch of five")
        assert np.array_equal(got[i].view(np.uint32), want[j].view(np.uint32)), (i, differ)


def test_chained_even_x_even_in_cl12_against_the_f64_kernel():
    n = 13
    even = [k for k in range(n + 1) if k % 2 == 0]
    odd = [k for k in range(n + 1) if k % 2 == 1]

    def build(B):                       # (odd * vector): an even left operand from a list, times an even right operand
        return (B.input(0, odd, n) * B.input(1, [1], n)) * B.input(2, even, n)
    rng = np.random.default_rng(1313)
    rows = {0: rows_of(n, odd, 1, rng, np.float32), 1: rows_of(n, [1], 1, rng, np.float32), 2: rows_of(n, even, 1, rng, np.float32)}
    rows64 = {s: r.astype(np.float64) for s, r in rows.items()}
    got, mask, spec = hip_eval_batch(build, n, rows, 1, dtype=ga.F32)
    assert len(spec.launches()) == 1 and "k_gp_mfma32p<false,12,false,true>" in spec.launches()[0], spec.launches()
    assert "even x even in Cl(12)" in spec.launches()[0], spec.launches()
    want, wmask, spec64 = hip_eval_batch(build, n, rows64, 1, dtype=ga.F64)
    assert mask == wmask and any("k_gp_mfma16x4<double,false,12," in l for l in spec64.launches()), spec64.launches()
    og = [k for k in range(n + 1) if (wmask >> k) & 1]
    # the left operand of the dense product, for the bound: the list product alone, in f64
    ax, axmask, _ = hip_eval_batch(lambda B: B.input(0, odd, n) * B.input(1, [1], n), n, {0: rows64[0], 1: rows64[1]}, 1, dtype=ga.F64)
    ag = [k for k in range(n + 1) if (axmask >> k) & 1]
    S = abs_terms_bound(n, row_to_bits(n, ag, ax[0]), row_to_bits(n, even, rows64[2][0]))
    bound = 4 * 2.0 ** -23 * bits_to_row(n, og, S) + 1e-300
    err = np.abs(got[0].astype(np.float64) - want[0])
    print(f"chained <false,12,false,true>: max err / bound = {float((err / bound).max()):.4f}, max |want| = {float(np.abs(want).max()):.3f}")
    assert np.abs(want).max() > 1.0     # a real product, not zeros
    assert np.all(err <= bound), float((err / bound).max())
