"""Register budget of the two kernels of gaast_hip_linmap_matrix_vjp (k_linmap_outer_sum, k_linmap_minor_contract), read from
the gfx950 code object inside libgaast_hip.so as test_kernel_resources.py reads the hot kernels' (no GPU needed).

Both instantiations of each (f32 / f64) exist, spill no register (no scratch memory) and leave at least four waves per SIMD;
the outer sum declares no LDS at all (its operands go from the rows straight into the matrix cores' registers)."""
import pytest

from test_kernel_resources import kernels  # noqa: F401  (the module-scoped fixture that parses the code object)


@pytest.mark.parametrize("ty", ["float", "double"])
@pytest.mark.parametrize("kernel", ["k_linmap_outer_sum", "k_linmap_minor_contract"])
def test_matrix_vjp_kernels_use_no_scratch(kernels, kernel, ty):  # noqa: F811
    hits = {k: v for k, v in kernels.items() if k.startswith(f"{kernel}<{ty}>")}
    assert len(hits) == 1, sorted(k for k in kernels if "linmap" in k)
    for name, k in hits.items():
        regs = -(-k["vgpr"] // 8) * 8
        print(name, k)
        assert k["spill"] == 0 and k["sgpr_spill"] == 0, (name, k)
        assert regs * 4 <= 512, (name, k, f"{regs} registers: fewer than 4 waves per SIMD")
        if kernel == "k_linmap_outer_sum":
            assert k["lds"] == 0, (name, k)
