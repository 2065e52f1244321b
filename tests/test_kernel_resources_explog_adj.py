"""Register budget of k_exp_log_adj (the stand-alone exp / log adjoint kernel), read from the gfx950 code object inside
libgaast_hip.so as test_kernel_resources.py reads the hot kernels' (no GPU needed).

Each of the four instantiations (f32 / f64, exp / log) spills no vector register, declares no static LDS (its staging buffer
is dynamic) and leaves at least four waves per SIMD."""
import pytest

from test_kernel_resources import kernels  # noqa: F401  (the module-scoped fixture that parses the code object)


@pytest.mark.parametrize("ty", ["float", "double"])
def test_exp_log_adjoint_kernel_does_not_spill(kernels, ty):  # noqa: F811
    hits = {k: v for k, v in kernels.items() if k.startswith(f"k_exp_log_adj<{ty},")}
    assert len(hits) == 2, sorted(kernels)[:20]
    for name, k in hits.items():
        regs = -(-k["vgpr"] // 8) * 8
        assert k["spill"] == 0, (name, k)
        assert k["lds"] == 0, (name, k)
        assert regs * 4 <= 512, (name, k, f"{regs} registers: fewer than 4 waves per SIMD")
