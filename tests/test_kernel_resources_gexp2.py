"""Register and LDS budget of k_mv_gexp_jvp<T, N> and k_mv_gexp_adj2<T, N> (the second-order pair of the general exponential,
kernels_gexp.hip.hpp), read from the gfx950 code object inside libgaast_hip.so by the reader of test_kernel_resources_gexp.py (no
GPU needed).

All 24 instantiations exist, use no scratch memory and spill no register.  Both declare their LDS statically, as the kernel header
states it: k_mv_gexp_jvp 6 x 256 + 128 elements of T and four ints; k_mv_gexp_adj2 36 x 256 + 128 elements and four ints -- 74768
bytes in f64, above 64 KiB but within the 80 KiB that lets two workgroups share a CU's 160 KiB.  The VGPR counts are recorded
(printed), not bounded."""
import pytest

from test_kernel_resources_gexp import _one, gexp_kernels  # noqa: F401  (the module-scoped fixture that reads the code object)

ROWS = {"k_mv_gexp_jvp": 6, "k_mv_gexp_adj2": 36}


@pytest.mark.parametrize("kernel", sorted(ROWS))
@pytest.mark.parametrize("ty", ["float", "double"])
@pytest.mark.parametrize("n", [2, 4, 8, 16, 32, 64])
def test_no_scratch_no_spills_and_the_stated_lds(gexp_kernels, kernel, ty, n):  # noqa: F811
    name, k = _one(gexp_kernels, kernel, ty, n)
    print("RESOURCES", name, k)   # the record: VGPRs of every instantiation
    assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)
    elem = 4 if ty == "float" else 8
    assert k["lds"] == (ROWS[kernel] * 256 + 128) * elem + 16, (name, k)
    assert k["lds"] <= 80 * 1024, "two workgroups per CU"


def test_the_new_names_do_not_match_the_prefixes_of_the_first_order_kernels(gexp_kernels):  # noqa: F811
    """test_kernel_resources_gexp.py finds its kernels by `k_mv_gexp<` and `k_mv_gexp_adj<`"""
    new = [k for k in gexp_kernels if k.startswith("k_mv_gexp_jvp<") or k.startswith("k_mv_gexp_adj2<")]
    assert len(new) == 24
    assert not any(k.startswith("k_mv_gexp<") or k.startswith("k_mv_gexp_adj<") for k in new)
