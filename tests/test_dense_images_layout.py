"""The operand images of the dense-product kernels on the CPU: a stand-alone program over the one header that states them
(gaast_amd/csrc/device/dense_images.hip.hpp), compiled with -fsanitize=address,undefined.  See tests/cpp/dense_images_driver.cpp
for what is checked."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_positions_tables_and_geometry_of_every_dense_family(tmp_path):
    exe = tmp_path / "dense_images_asan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "gaast_amd", "csrc", "device"), os.path.join(ROOT, "tests", "cpp", "dense_images_driver.cpp")]
    subprocess.run(cmd + ["-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.strip().endswith("ALL OK")
