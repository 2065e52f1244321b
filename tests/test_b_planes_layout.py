"""The quad-plane B image of k_gp_mfma32p<false, 12> and the address algebra of its step loop, on the CPU: a stand-alone
program over the one header that states the layout (gaast_amd/csrc/device/mfma32p_b_planes.hip.hpp) and the plan builder,
compiled with -fsanitize=address,undefined.  See tests/cpp/b_planes_driver.cpp for what is checked."""
import os
import subprocess

from helpers import plan_sources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_quad_plane_addresses_hold_the_words_of_every_step(tmp_path):
    csrc = os.path.join(ROOT, "gaast_amd", "csrc")
    exe = tmp_path / "b_planes_asan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(csrc, "device"), "-I", os.path.join(csrc, "common"), "-I", os.path.join(csrc, "host"),
           os.path.join(ROOT, "tests", "cpp", "b_planes_driver.cpp")]
    cmd += plan_sources(csrc)
    subprocess.run(cmd + ["-o", str(exe)], check=True, cwd=csrc)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.strip().endswith("ALL OK")
