"""The kernel cache without a GPU: its store (gaast_amd/csrc/device/jit_cache.cpp: SHA-256, key, file format, atomic
replacement) compiled with g++ -fsanitize=address,undefined and driven by tests/cpp/jit_cache_driver.cpp, and the two C-ABI
entry points through ctypes.  The GPU side is tests/test_gpu_jit_cache.py."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    device = os.path.join(ROOT, "gaast_amd", "csrc", "device")
    exe = tmp_path_factory.mktemp("jit_cache_driver") / "jit_cache_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", device, os.path.join(ROOT, "tests", "cpp", "jit_cache_driver.cpp"),
                    os.path.join(device, "jit_cache.cpp"), "-o", str(exe)], check=True)

    def run(*args):
        r = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-4000:]
        return r.stdout
    run.exe = str(exe)
    return run


def test_sha256_matches_the_fips_180_vectors(driver):
    driver("sha")


def test_key_changes_with_every_field_and_with_a_byte_moved_between_fields(driver):
    driver("key")


def test_store_then_load_round_trips_payloads_up_to_beyond_1_mib(driver, tmp_path):
    driver("roundtrip", tmp_path)
    assert all(f.endswith(".gaastco") for f in os.listdir(tmp_path)), os.listdir(tmp_path)


def test_truncated_flipped_and_foreign_files_are_rejected_and_a_store_repairs_them(driver, tmp_path):
    driver("reject", tmp_path)
    assert len(os.listdir(tmp_path)) == 1


def test_missing_and_read_only_directories_fail_without_throwing(driver, tmp_path):
    driver("baddirs", tmp_path)


def test_two_processes_storing_one_key_leave_one_complete_file(driver, tmp_path):
    """the ranks of a launch: both write <key>.gaastco at once; each writes a payload of ONE repeated byte, so a file pieced
    together from two writers fails the check of its contents even where its hash were right"""
    size = 3 << 20
    for round_ in range(32):
        kids = [subprocess.Popen([driver.exe, "store", str(tmp_path), str(fill), str(size)], stdout=subprocess.PIPE, text=True)
                for fill in (2 * round_ + 1, 2 * round_ + 2)]
        for k in kids:
            out, _ = k.communicate(timeout=300)
            assert k.returncode == 0, out
        name = driver("verify", tmp_path, size).split()[0]
        assert os.listdir(tmp_path) == [name], os.listdir(tmp_path)


# ---- the C ABI, without a GPU ------------------------------------------------------------------------------------------
# (a child process each: the directory is a setting of the process, and the counters are the process's)
def _child(code, *args):
    r = subprocess.run([sys.executable, "-c", code, *map(str, args)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_set_dir_accepts_a_fresh_directory_null_and_empty_and_refuses_a_file(tmp_path):
    plain = tmp_path / "plain"
    plain.write_text("x")
    out = _child("""
import ctypes as C, os, sys
import gaast_amd
L = gaast_amd.lib()
fresh, plain = sys.argv[1].encode(), sys.argv[2].encode()
assert not os.path.exists(fresh)
assert L.gaast_hip_jit_cache_set_dir(fresh) == 0
assert os.path.isdir(fresh)
assert L.gaast_hip_jit_cache_set_dir(fresh) == 0          # already there
assert L.gaast_hip_jit_cache_set_dir(None) == 0
assert L.gaast_hip_jit_cache_set_dir(b"") == 0
assert L.gaast_hip_jit_cache_set_dir(plain) == 6, "GAAST_ERR_INVALID_ARGUMENT"
assert b"not a directory" in L.gaast_hip_last_error()
assert L.gaast_hip_jit_cache_set_dir(fresh + b"/a/b") == 6  # only the last component is created
assert not os.path.exists(fresh + b"/a")
# the Python surface
gaast_amd.jit_cache_dir(sys.argv[1])
gaast_amd.jit_cache_dir(None)
try:
    gaast_amd.jit_cache_dir(sys.argv[2])
except gaast_amd.GaastError as e:
    assert e.status_name == "INVALID_ARGUMENT"
else:
    raise AssertionError("a regular file was accepted")
assert os.listdir(fresh) == []
print("OK")
""", tmp_path / "fresh", plain)
    assert out.strip().endswith("OK")


def test_stats_report_six_zero_counters_before_any_program():
    out = _child("""
import ctypes as C
import gaast_amd
L = gaast_amd.lib()
assert L.gaast_hip_jit_cache_stats(None, 0) == 6
buf = (C.c_int64 * 8)(*[-1] * 8)
assert L.gaast_hip_jit_cache_stats(buf, 3) == 6
assert list(buf) == [0, 0, 0, -1, -1, -1, -1, -1], list(buf)
assert L.gaast_hip_jit_cache_stats(buf, 8) == 6
assert list(buf) == [0] * 6 + [-1, -1], list(buf)
assert gaast_amd.jit_cache_stats() == dict(compiled=0, memory_hits=0, disk_hits=0, disk_stores=0, disk_rejected=0, live_modules=0)
print("OK")
""")
    assert out.strip().endswith("OK")


def test_header_documents_the_layout_the_store_writes(driver, tmp_path):
    """include/gaast_hip.h is what other hosts read the format from: the offsets there are the offsets in a stored file"""
    import hashlib
    import re
    import struct
    header = open(os.path.join(ROOT, "include", "gaast_hip.h")).read()
    offs = [int(m) for m in re.findall(r"^ \*     offset +(\d+) ", header, flags=re.M)]
    assert offs == [0, 8, 12, 44, 76, 84, 116], offs
    size = 1000
    subprocess.run([driver.exe, "store", str(tmp_path), "7", str(size)], check=True, capture_output=True)
    (name,) = os.listdir(tmp_path)
    data = open(tmp_path / name, "rb").read()
    assert data[0:8] == b"GAASTCO\0" and struct.unpack_from("<I", data, 8)[0] == 1
    assert data[12:44].rstrip(b"\0") == b"0123456789ab"
    assert data[44:76].hex() + ".gaastco" == name
    assert struct.unpack_from("<Q", data, 76)[0] == size == len(data) - 116
    assert data[84:116] == hashlib.sha256(data[116:]).digest() and data[116:] == b"\x07" * size
