"""The kernel cache on the GPU (include/gaast_hip.h: gaast_hip_jit_cache_*): a cold process compiles and stores, a warm one
loads the very code objects and computes the very bits under the very launch names, damaged files are replaced, programs of
one process share their modules, and GAAST_FLAG_DEBUG_JIT_FAILS sees neither level.

Every stage is a fresh process (tests/jit_cache_worker.py) -- one at a time, each under its own time limit.  Once one of them
has died abnormally no further process is started by this file."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "jit_cache_worker.py")
STAGE_TIMEOUT_S = 420
_died = []


def _stage(*args, cwd=None):
    if _died:
        pytest.fail(f"not started: an earlier stage died abnormally ({_died[0]})")
    try:
        r = subprocess.run([sys.executable, WORKER, *map(str, args)], capture_output=True, text=True, timeout=STAGE_TIMEOUT_S, cwd=cwd)
    except subprocess.TimeoutExpired:
        _died.append(f"{args}: time limit")
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _died.append(f"{args}: exit status {r.returncode}")
    assert r.returncode == 0, f"exit status {r.returncode}\n" + r.stdout[-3000:] + r.stderr[-6000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(args, json.dumps(out.get("stats", out))[:2000])
    return out


def _cache_files(path):
    names = sorted(os.listdir(path))
    assert all(len(n) == 64 + len(".gaastco") and n.endswith(".gaastco") for n in names), names   # (and no temporary file)
    return names


def test_cold_then_warm_then_damaged_then_repaired(tmp_path):
    cache = tmp_path / "cache"
    # 1: cold
    cold = _stage("run", cache)
    s = cold["stats"]
    assert s["compiled"] > 0 and s["disk_hits"] == 0 and s["disk_rejected"] == 0, s
    assert s["disk_stores"] == s["compiled"], s
    files = _cache_files(cache)
    assert len(files) == s["compiled"], (files, s)
    # what the programs are supposed to exercise: both builds of the shared-rotor sandwich, slabs in LDS, the chain kernels
    labels = cold["launches"]
    assert cold["per_program"]["cl41s"]["compiled"] == 2 and "fused multiply-adds" in labels["cl41s"][0], labels["cl41s"]
    assert "slab in LDS" in labels["vinv8"][0], labels["vinv8"]
    assert any("ast_jit" in l for l in labels["proj12"]), labels["proj12"]
    for name in ("sand9g1x", "cfg1_8x"):
        assert cold["per_program"][name]["compiled"] + cold["per_program"][name]["memory_hits"] >= 1, (name, cold["per_program"][name], labels[name])
    # 2: warm from the directory
    warm = _stage("run", cache)
    w = warm["stats"]
    assert w["compiled"] == 0 and w["disk_stores"] == 0 and w["disk_rejected"] == 0, w
    assert w["disk_hits"] == s["compiled"], (w, s)
    assert warm["launches"] == cold["launches"]
    assert warm["rows"] == cold["rows"]
    assert _cache_files(cache) == files
    # 3: one file cut short, one payload byte flipped in another
    cut, flipped = cache / files[0], cache / files[-1]
    data = cut.read_bytes()
    cut.write_bytes(data[:116 + (len(data) - 116) // 2])
    data = bytearray(flipped.read_bytes())
    data[116 + (len(data) - 116) // 3] ^= 0x10
    flipped.write_bytes(bytes(data))
    hurt = _stage("run", cache)
    h = hurt["stats"]
    assert h["disk_rejected"] == 2 and h["compiled"] == 2 and h["disk_stores"] == 2, h
    assert h["disk_hits"] == s["compiled"] - 2, (h, s)
    assert hurt["launches"] == cold["launches"]
    assert hurt["rows"] == cold["rows"]
    assert _cache_files(cache) == files
    # 4: the two files were replaced by good ones
    again = _stage("run", cache)
    a = again["stats"]
    assert a["compiled"] == 0 and a["disk_rejected"] == 0 and a["disk_hits"] == s["compiled"], a
    assert again["rows"] == cold["rows"]


def test_two_programs_of_one_expression_share_their_modules_until_the_last_is_destroyed():
    report = _stage("share")
    assert set(report) == {"cl41s", "sand9g1x", "vinv8"} and all(r["modules"] >= 1 for r in report.values()), report


def test_debug_jit_fails_finds_neither_cache_level(tmp_path):
    cold = _stage("jitfails", "-")
    assert cold["stats"] == dict(compiled=0, memory_hits=0, disk_hits=0, disk_stores=0, disk_rejected=0, live_modules=0), cold["stats"]
    for name, labels in cold["launches"].items():
        assert not any("ast_jit" in l or "gaast_chain" in l for l in labels), (name, labels)
    cache = tmp_path / "cache"
    filled = _stage("run", cache)["stats"]
    assert filled["disk_stores"] == filled["compiled"] > 0
    warm = _stage("jitfails", cache)
    assert warm["warm"]["disk_hits"] == filled["compiled"] and warm["warm"]["compiled"] == 0, warm["warm"]
    assert warm["warm"]["live_modules"] > 0
    assert warm["stats"] == warm["warm"], (warm["warm"], warm["stats"])      # no counter moved under the flag
    assert warm["launches"] == cold["launches"]
    assert warm["rows"] == cold["rows"]


def test_without_a_directory_nothing_is_written(tmp_path):
    cwd = tmp_path / "cwd"
    cwd.mkdir()
    out = _stage("run", "-", cwd=cwd)
    s = out["stats"]
    assert s["compiled"] > 0 and s["disk_hits"] == 0 and s["disk_stores"] == 0 and s["disk_rejected"] == 0, s
    assert out["new_files_in_cwd"] == []
    assert [p for p in tmp_path.rglob("*") if p != cwd] == []
