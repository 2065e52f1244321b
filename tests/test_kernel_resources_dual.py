"""Register budget of k_dual (the complements' kernel, kernels_exact.hip.hpp), read from the gfx950 code object inside
libgaast_hip.so as test_kernel_resources.py reads the hot kernels' (no GPU needed).

Both instantiations exist, spill no register (no scratch memory), declare no LDS and stay a small, HBM-bound kernel: the VGPR
counts are recorded here (18 for both value types on the day they were written) and bounded by 32, far inside the eight waves per SIMD
an element-wise kernel wants."""
import pytest

from test_kernel_resources import kernels  # noqa: F401  (the module-scoped fixture that parses the code object)


@pytest.mark.parametrize("ty", ["float", "double"])
def test_k_dual_uses_no_scratch(kernels, ty):  # noqa: F811
    hits = {k: v for k, v in kernels.items() if k.startswith(f"k_dual<{ty}>")}
    assert len(hits) == 1, sorted(k for k in kernels if "dual" in k)
    for name, k in hits.items():
        print(name, k)
        assert k["spill"] == 0 and k["sgpr_spill"] == 0, (name, k)
        assert k.get("scratch", 0) == 0 and k["lds"] == 0, (name, k)
        assert k["vgpr"] <= 32, (name, k)
