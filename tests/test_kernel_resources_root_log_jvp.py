"""Register and LDS budget of k_mv_gsqrt_jvp<T, N> and k_mv_jvp_glog<T, N> (the tangents of the general square root and logarithm,
kernels_gsqrt.hip.hpp / kernels_glog.hip.hpp), read from the gfx950 code object inside libgaast_hip.so as
test_kernel_resources_glog.py reads the first-order kernels' (no GPU needed).

All 24 instantiations exist, use no scratch memory and spill no register, vector or scalar.  Each holds a row of N values of T per
lane through one elimination at a time; at N = 64 both must still fit the two waves per SIMD their __launch_bounds__(256, 2) asks for
(at most 256 of the 512 registers per lane) in both dtypes.  Their static LDS is their adjoint sibling's, byte for byte:
gsqrt_detail::Shared for the root's tangent, and beside it glog_detail::ExtraAdj (the chain X_1 ... X_16) for the logarithm's.  The
counts are recorded (printed; DESIGN.md sections 16.1 and 17.1)."""
import re
import struct
import subprocess

import pytest

from gaast_amd import _lib
from test_kernel_resources import CXXFILT, READELF

KERNELS = ["k_mv_gsqrt_jvp", "k_mv_jvp_glog"]
SIBLING = {"k_mv_gsqrt_jvp": "k_mv_gsqrt_adj", "k_mv_jvp_glog": "k_mv_glog_adj"}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    data = open(_lib.LIB_PATH, "rb").read()
    i = data.find(b"__CLANG_OFFLOAD_BUNDLE__")
    assert i >= 0, "no offload bundle in the library"
    n = struct.unpack_from("<Q", data, i + 24)[0]
    off, co = i + 32, None
    for _ in range(n):
        o, sz, tl = struct.unpack_from("<QQQ", data, off)
        off += 24
        triple = data[off:off + tl].decode()
        off += tl
        if "gfx950" in triple:
            co = data[i + o:i + o + sz]
    assert co, "no gfx950 code object"
    path = tmp_path_factory.mktemp("co_root_log_jvp") / "gaast.co"
    path.write_bytes(co)
    notes = subprocess.run([READELF, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
    out = {}
    for block in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if not any(k in name for k in KERNELS + list(SIBLING.values())):
            continue
        field = lambda f: int(re.search(r"\.%s:\s+(\d+)" % f, block).group(1))
        out[name] = dict(vgpr=field("vgpr_count"), agpr=int(block.split()[0]), sgpr=field("sgpr_count"), spill=field("vgpr_spill_count"),
                         sgpr_spill=field("sgpr_spill_count"), lds=field("group_segment_fixed_size"), scratch=field("private_segment_fixed_size"))
    names = subprocess.run([CXXFILT], input="\n".join(out), capture_output=True, text=True, check=True).stdout.split("\n")
    return {d.replace("void gaast::", "").split("(")[0]: v for d, v in zip(names, out.values())}


def _one(kernels, kernel, ty, n):
    hits = {k: v for k, v in kernels.items() if k.startswith(f"{kernel}<{ty},") and k.split(",")[1].strip().startswith(f"{n}>")}
    assert len(hits) == 1, sorted(kernels)
    return next(iter(hits.items()))


def test_all_24_instantiations_exist(kernels):
    assert len([k for k in kernels if k.split("<")[0] in KERNELS]) == 24, sorted(kernels)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("ty", ["float", "double"])
@pytest.mark.parametrize("n", [2, 4, 8, 16, 32, 64])
def test_no_scratch_no_spills_and_the_lds_of_the_adjoint_sibling(kernels, kernel, ty, n):
    name, k = _one(kernels, kernel, ty, n)
    print("RESOURCES", name, k)   # the record: VGPRs of every instantiation
    assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)
    elem = 4 if ty == "float" else 8
    shared = (4 * 256 + 128) * elem + 32                                                   # gsqrt_detail::Shared<T>
    extra = 16 * elem + 32 + 16 * 256 * elem if kernel == "k_mv_jvp_glog" else 0           # glog_detail::ExtraAdj<T>
    assert k["lds"] == shared + extra, (name, k)
    assert k["lds"] <= _one(kernels, SIBLING[kernel], ty, n)[1]["lds"]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("ty", ["float", "double"])
def test_at_64_blades_both_fit_two_waves_per_simd(kernels, kernel, ty):
    name, k = _one(kernels, kernel, ty, 64)
    regs = -(-k["vgpr"] // 8) * 8          # .vgpr_count is the unified total (arch + accumulation registers); granule: 8
    assert regs * 2 <= 512, (name, k)
