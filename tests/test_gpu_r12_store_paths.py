"""The two store paths and the zero-C start of k_gp_mfma32p<false, 12> (n = 12, f32).

The launcher picks, per launch, how the kernel writes its results (plan.hpp: dense_whole_row_stores; the flags themselves are checked on
the CPU in tests/test_dense_store_flags.py):
  * whole rows -- every blade has a place in the result row, no reordering sign, nothing accumulated: the lane's 16 out_map words are
    read once per launch and kept as byte offsets, each result is one store from a uniform row base;
  * the general put() -- out_map words read per item, absent blades skipped, reordering signs, read-modify-write under beta.
The item's first MFMA takes a zero C operand instead of a zeroed accumulator.  None of this may move a bit: the sums are the same
fused multiply-add chains in the same order (tests/test_gpu_r12_bits.py pins them).
"""
import os

import numpy as np
import pytest

import gaast_amd as ga
from helpers import abs_terms_bound, bits_to_row, full_grades, hip_eval_batch, n_choose_k, row_to_bits, rows_of
from layouts import place, place_out

pytestmark = pytest.mark.gpu

N = 12
FG = full_grades(N)
KERNEL = "k_gp_mfma32p<false,12>"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "r12_bits.npz")


def _full(B):
    return B.input(0, FG, N) * B.input(1, FG, N)


def _runs_the_kernel(spec):
    return any(l.startswith("product_dense_mfma[") and l.split(" :: ")[-1].startswith(KERNEL) for l in spec.launches())


@pytest.fixture(scope="module")
def five():
    """a batch of five: the three items of the golden file's `plain` case (tests/test_gpu_r12_bits.py: seed 1201) and two more;
    rows (read-only), the full product's result rows, the spec"""
    rng = np.random.default_rng(1201)
    rows = {0: rows_of(N, FG, 3, rng, np.float32), 1: rows_of(N, FG, 3, rng, np.float32)}
    extra = np.random.default_rng(1207)
    rows = {s: np.ascontiguousarray(np.concatenate([r, rows_of(N, FG, 2, extra, np.float32)])) for s, r in rows.items()}
    got, _, spec = hip_eval_batch(_full, N, rows, 5, dtype=ga.F32)
    assert _runs_the_kernel(spec), spec.launches()
    for r in rows.values():
        r.setflags(write=False)
    got.setflags(write=False)
    return rows, got, spec


def test_whole_rows_into_a_fresh_result_and_into_a_strided_offset_view(five):
    rows, fresh, spec = five
    want = np.load(GOLDEN)["plain"]
    assert np.abs(want).max() > 1.0
    assert np.array_equal(fresh[:3].view(np.uint32), want.view(np.uint32)), int((fresh[:3].view(np.uint32) != want.view(np.uint32)).sum())
    # the same launch form into rows one element off a 16-byte boundary, 16 bytes and more apart, canaries all around
    placed = {s: place(rows[s], "contig", ga.F32, N, FG) for s in range(2)}
    out = place_out(5, 1 << N, "shift_pad16", ga.F32, N, FG)
    spec.eval_batch([placed[0].mv, placed[1].mv], 5, out=out.mv)
    view = out.rows()
    for p in (placed[0], placed[1], out):
        p.check()
    differ = int((view.view(np.uint32) != fresh.view(np.uint32)).sum())
    print(f"strided, offset result view: {differ} of {view.size} words differ from the fresh result")
    assert np.array_equal(view.view(np.uint32), fresh.view(np.uint32)), differ


@pytest.mark.parametrize("k", [6, 5])
def test_projected_product_takes_the_general_put_and_keeps_the_bits(five, k):
    """(a * b).g(k): the blades of every other grade have out_map words < 0"""
    rows, full, _ = five
    got, mask, spec = hip_eval_batch(lambda B: _full(B).g(k), N, dict(rows), 5, dtype=ga.F32)
    assert _runs_the_kernel(spec), spec.launches()
    assert mask == 1 << k
    first = sum(n_choose_k(N, j) for j in range(k))
    want = full[:, first:first + n_choose_k(N, k)]
    assert got.shape == want.shape and np.abs(want).max() > 1.0
    differ = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"grade {k}: {differ} of {got.size} words differ from the full product's components")
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), differ


def test_accumulating_product_against_the_f64_kernel():
    """a * b + c * d: the second dense product adds into the row the first one wrote (beta = 1: the general put(); the first takes the
    whole-row path).  Bound, per component: 4 eps sum|terms| for each product (tests/test_gpu_dense_oracle.py) and one rounding of
    the sum, at most eps / 2 of |result| <= the two sums of |terms| -- 5 eps (S_ab + S_cd), as that file bounds a sum of two products."""
    batch = 5
    rng = np.random.default_rng(1231)
    rows = {s: rows_of(N, FG, batch, rng, np.float32) for s in range(4)}
    rows64 = {s: r.astype(np.float64) for s, r in rows.items()}

    def build(B):
        return B.input(0, FG, N) * B.input(1, FG, N) + B.input(2, FG, N) * B.input(3, FG, N)
    got, mask, spec = hip_eval_batch(build, N, rows, batch, dtype=ga.F32)
    assert sum(l.startswith("product_dense_mfma[") and l.split(" :: ")[-1].startswith(KERNEL) for l in spec.launches()) == 2, spec.launches()
    want, wmask, spec64 = hip_eval_batch(build, N, rows64, batch, dtype=ga.F64)
    assert mask == wmask and sum("k_gp_mfma16x4<double,false,12," in l for l in spec64.launches()) == 2, spec64.launches()
    assert np.abs(want).max() > 1.0
    worst = 0.0
    for i in range(batch):
        S = sum(abs_terms_bound(N, row_to_bits(N, FG, rows64[a][i]), row_to_bits(N, FG, rows64[b][i])) for a, b in ((0, 1), (2, 3)))
        bound = 5 * 2.0 ** -23 * bits_to_row(N, FG, S) + 1e-300
        err = np.abs(got[i].astype(np.float64) - want[i])
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (i, float((err / bound).max()))
    print(f"a * b + c * d, f32 against f64: max err / bound = {worst:.4f}")


def test_later_items_of_a_persistent_workgroup_on_the_whole_row_path(five):
    """batch 2 * 2 * CUs + 3: every workgroup takes two items, three take a third; the register-held offsets and the zero-C start of
    every item after the first must give the rows a batch of five gives (one item per workgroup)"""
    import torch
    rows5, want, _ = five
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    batch = 2 * cus * 2 + 3
    pick = [0, batch // 3, batch // 2, (3 * batch) // 4 + 1, batch - 1]
    rng = np.random.default_rng(1241)
    rows = {s: rows_of(N, FG, batch, rng, np.float32) for s in range(2)}
    for s in range(2):
        rows[s][pick] = rows5[s]
    got, _, spec = hip_eval_batch(_full, N, rows, batch, dtype=ga.F32)
    assert _runs_the_kernel(spec), spec.launches()
    for j, i in enumerate(pick):
        differ = int((got[i].view(np.uint32) != want[j].view(np.uint32)).sum())
        print(f"row {i} of {batch}: {differ} of {got.shape[1]} words differ from the batch of five")
        assert np.array_equal(got[i].view(np.uint32), want[j].view(np.uint32)), (i, differ)
    # and a row that is not among the five is not one of them (the rows above were really computed in place)
    assert not np.array_equal(got[1].view(np.uint32), want[0].view(np.uint32))
