"""Register budget of k_mv_inverse<T, N> (the general inverse's kernel, kernels_inverse.hip.hpp), read from the gfx950 code object
inside libgaast_hip.so as test_kernel_resources.py reads the hot kernels' (no GPU needed).

All twelve instantiations exist and spill no register (no scratch memory).  A lane holds a row of N values of T in registers, so the
VGPR count grows with N; the bound is 256 -- two waves per SIMD, which is what a kernel bound by its vector ALUs and cross-lane
traffic needs -- tightened per instantiation to what was observed on the day this was written (OBSERVED: 33 ... 99 VGPRs in f32,
45 ... 172 in f64), plus modest headroom.  The kernel declares its LDS statically: 256 + 128 elements of T."""
import pytest

from test_kernel_resources import kernels  # noqa: F401  (the module-scoped fixture that parses the code object)

# (type, N) -> VGPR bound: the count observed on the day this was written plus about a tenth, never above 256
OBSERVED = {("float", 2): 33, ("double", 2): 45, ("float", 4): 40, ("double", 4): 55, ("float", 8): 48, ("double", 8): 64,
            ("float", 16): 53, ("double", 16): 83, ("float", 32): 70, ("double", 32): 120, ("float", 64): 99, ("double", 64): 172}
BOUNDS = {k: min(256, v + max(6, v // 10)) for k, v in OBSERVED.items()}


@pytest.mark.parametrize("ty", ["float", "double"])
@pytest.mark.parametrize("n", [2, 4, 8, 16, 32, 64])
def test_k_mv_inverse_uses_no_scratch(kernels, ty, n):  # noqa: F811
    hits = {k: v for k, v in kernels.items() if k.startswith(f"k_mv_inverse<{ty},") and k.split(",")[1].strip().startswith(f"{n}>")}
    assert len(hits) == 1, sorted(k for k in kernels if "inverse" in k)
    for name, k in hits.items():
        print(name, k)
        assert k["spill"] == 0 and k["sgpr_spill"] == 0, (name, k)
        assert k.get("scratch", 0) == 0, (name, k)
        assert k["lds"] == 384 * (4 if ty == "float" else 8), (name, k)
        assert k["vgpr"] <= BOUNDS[(ty, n)] <= 256, (name, k)
