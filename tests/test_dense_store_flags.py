"""The launch-time forms of k_gp_mfma32p<false, 12, *, *> -- whole-row result stores, a side staged without the sign xor -- follow
the words of the plan's maps, on the CPU: a stand-alone program over the plan builder and plan.hpp's dense_whole_row_stores, compiled
with -fsanitize=address,undefined.  See tests/cpp/dense_flags_driver.cpp for the programs and what is checked."""
import os
import subprocess

from helpers import plan_sources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_whole_row_and_sign_flags_follow_the_maps(tmp_path):
    csrc = os.path.join(ROOT, "gaast_amd", "csrc")
    exe = tmp_path / "dense_flags_asan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(csrc, "device"), "-I", os.path.join(csrc, "common"), "-I", os.path.join(csrc, "host"),
           os.path.join(ROOT, "tests", "cpp", "dense_flags_driver.cpp")]
    cmd += plan_sources(csrc)
    subprocess.run(cmd + ["-o", str(exe)], check=True, cwd=csrc)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.strip().endswith("ALL OK")
