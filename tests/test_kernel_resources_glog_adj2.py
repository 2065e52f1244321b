"""Register and LDS budget of k_mv_adj2_glog<T, N> (the second-order adjoint of the general logarithm, kernels_glog.hip.hpp), read from the
gfx950 code object inside libgaast_hip.so as test_kernel_resources_root_log_jvp.py reads the tangents' (no GPU needed).

All 12 instantiations exist, use no scratch memory and spill no register, vector or scalar.  Their static LDS is the three structs of
the kernel, byte for byte -- gsqrt_detail::Shared, glog_detail::ExtraAdj (the chain X_1 ... X_16) and glog_detail::ExtraAdj2 (the chain
t_1 ... t_16 and three parked values per lane) -- and at most 80 KiB, so that two workgroups fit the 160 KiB of a CU in f64 (four in
f32).  At N = 64 the kernel must still fit the two waves per SIMD its __launch_bounds__(256, 2) asks for (at most 256 of the 512
registers per lane) in both dtypes.  The counts are recorded (printed)."""
import re
import struct
import subprocess

import pytest

from gaast_amd import _lib
from test_kernel_resources import CXXFILT, READELF

KERNEL = "k_mv_adj2_glog"


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
    path = tmp_path_factory.mktemp("co_glog_adj2") / "gaast.co"
    path.write_bytes(co)
    notes = subprocess.run([READELF, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
    out = {}
    for block in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if KERNEL not in name:
            continue
        field = lambda f: int(re.search(r"\.%s:\s+(\d+)" % f, block).group(1))
        out[name] = dict(vgpr=field("vgpr_count"), agpr=int(block.split()[0]), sgpr=field("sgpr_count"), spill=field("vgpr_spill_count"),
                         sgpr_spill=field("sgpr_spill_count"), lds=field("group_segment_fixed_size"), scratch=field("private_segment_fixed_size"))
    names = subprocess.run([CXXFILT], input="\n".join(out), capture_output=True, text=True, check=True).stdout.split("\n")
    return {d.replace("void gaast::", "").split("(")[0]: v for d, v in zip(names, out.values())}


def _one(kernels, ty, n):
    hits = {k: v for k, v in kernels.items() if k.startswith(f"{KERNEL}<{ty},") and k.split(",")[1].strip().startswith(f"{n}>")}
    assert len(hits) == 1, sorted(kernels)
    return next(iter(hits.items()))


def test_all_12_instantiations_exist(kernels):
    assert len([k for k in kernels if k.split("<")[0] == KERNEL]) == 12, sorted(kernels)


@pytest.mark.parametrize("ty", ["float", "double"])
@pytest.mark.parametrize("n", [2, 4, 8, 16, 32, 64])
def test_no_scratch_no_spills_and_the_lds_of_the_three_structs(kernels, ty, n):
    name, k = _one(kernels, ty, n)
    print("RESOURCES", name, k)   # the record: VGPRs of every instantiation
    assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)
    elem = 4 if ty == "float" else 8
    shared = (4 * 256 + 128) * elem + 32                 # gsqrt_detail::Shared<T>
    extra = 16 * 256 * elem + 16 * elem + 32             # glog_detail::ExtraAdj<T>
    extra2 = (16 + 3) * 256 * elem                       # glog_detail::ExtraAdj2<T>
    assert k["lds"] == shared + extra + extra2, (name, k)
    assert k["lds"] <= 80 * 1024


@pytest.mark.parametrize("ty", ["float", "double"])
def test_at_64_blades_it_fits_two_waves_per_simd(kernels, ty):
    name, k = _one(kernels, ty, 64)
    regs = -(-k["vgpr"] // 8) * 8          # .vgpr_count is the unified total (arch + accumulation registers); granule: 8
    assert regs * 2 <= 512, (name, k)
