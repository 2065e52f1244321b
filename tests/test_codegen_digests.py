"""The plan builder's generated code, pinned byte for byte -- CPU only, no HIP.

tests/cpp/codegen_dump_driver.cpp lowers a fixed corpus with gaast::build_plan and writes every generated artifact of every step:
the hiprtc sources of gaast_jit (slab in registers / slabs in LDS) and gaast_chain, the k_ast_fused micro-op stream, and the tables
and settings built next to them.  Length and SHA-256 of each must equal tests/golden/codegen_digests.json (recorded by
tools/record_codegen_digests.py BEFORE a change to the generators).  The runtime compiles these strings and keys its compiled-code
cache by their hash: equal bytes are equal kernels."""
import glob
import hashlib
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "codegen_digests.json")

# what the corpus must reach inside the gaast_jit sources: form -> a line only that form emits
JIT_FORMS = {
    "direct rows, 256 threads": "if (item >= batch) return;",
    "input by span": "const VT* src0 = ",
    "span input, whole chunks": "*(VT*)(img + (el / ",
    "span input, chunks straddling rows": "img[((el + 0) / ",
    "span, guarded last chunk": "if (lane + ",
    "input by 128-byte lines": "const T* base = in",
    "input left to its lane": "  if (live) { const T* r = in",
    "output by span": "  if (full && so == ",
    "output span, whole chunks": "c = *(const VT*)(img + ",
    "output span, chunks straddling rows": "c[0] = img[((el + 0) / ",
    "output by 128-byte lines": "T* base = out + item0 * so",
    "output direct beside staged inputs": "  if (false && so == ",
    "operand read as 0.0 + x": " = T(0) + r[",
    "general coefficient": ") * T(0x",
    "exp": "cosh(t)",
    "log": "atanh(mm / ",
    "exp / log domain check": "atomicAdd(dom, 1ull)",
    "1 / s": " = T(1) / ",
    "sqrt, f32": "__builtin_sqrtf(",
    "sqrt, f64": "__builtin_sqrt(",
    "slabs in LDS": "__shared__ T slab[",
    "slabs in LDS, 16-byte pieces": "const bool fast = true && ",
    "slabs in LDS, too many pieces per thread": "const bool fast = false;",
}


def build_and_run(csrc, out_dir, exe):
    """Compile the driver against the plan sources under `csrc`, run it into out_dir; returns (digests, stdout)."""
    cmd = ["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(csrc, "device"), "-I", os.path.join(csrc, "common"), "-I", os.path.join(csrc, "host"),
           os.path.join(ROOT, "tests", "cpp", "codegen_dump_driver.cpp")]
    cmd += [os.path.join(csrc, f) for f in ("host/expr.cpp", "host/c_api_host.cpp", "host/wire.cpp")]
    cmd += sorted(glob.glob(os.path.join(csrc, "device", "plan*.cpp")))
    subprocess.run(cmd + ["-o", str(exe)], check=True)
    os.makedirs(out_dir, exist_ok=True)
    run = subprocess.run([str(exe), str(out_dir)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    digests = {}
    for name in sorted(os.listdir(out_dir)):
        with open(os.path.join(out_dir, name), "rb") as f:
            data = f.read()
        digests[name] = [len(data), hashlib.sha256(data).hexdigest()]
    return digests, run.stdout


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("codegen")
    csrc = os.environ.get("GAAST_CODEGEN_CSRC", os.path.join(ROOT, "gaast_amd", "csrc"))   # (another checkout's sources, for A/B)
    digests, stdout = build_and_run(csrc, tmp / "out", tmp / "codegen_dump")
    return digests, stdout, tmp / "out"


def test_generated_code_and_tables_match_the_recorded_digests(dumped):
    digests, _, _ = dumped
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(digests) == sorted(want), (sorted(set(want) - set(digests))[:10], sorted(set(digests) - set(want))[:10])
    wrong = [k for k in sorted(want) if digests[k] != want[k]]
    assert not wrong, "%d of %d artifacts differ: %s" % (len(wrong), len(want), wrong[:12])


def test_corpus_reaches_every_form_of_the_generators(dumped):
    _, stdout, out = dumped
    fused = re.findall(r"FUSED form=(\w+) jit_only=(\d) trial=(\d) general=(\d+)", stdout)
    assert {f[0] for f in fused} == {"reg", "lds", "interp"}
    assert {(f[0], f[1]) for f in fused} >= {("reg", "0"), ("reg", "1")}          # jit_only
    assert {(f[0], f[2]) for f in fused} >= {("reg", "0"), ("reg", "1")}          # jit_reg_trial
    assert any(f[0] == "interp" and int(f[3]) > 0 for f in fused)                 # LINE_MACS_GEN rows
    chains = re.findall(r"CHAIN single=(\d) xreg=(\d) sorted=(\d) fmt1=(\d) split=(\d+)", stdout)
    assert {c[0] for c in chains} == {"0", "1"}
    assert {c[1] for c in chains} == {"0", "1"}
    assert {c[2] for c in chains} == {"0", "1"}
    assert {c[3] for c in chains} == {"0", "1", "2", "3", "4"}    # narrow (global, LDS), wide, sign-sorted (LDS, global)
    assert {c[4] == "1" for c in chains} == {True, False}
    sources = []
    for name in sorted(os.listdir(out)):
        if name.endswith(".fused_jit_source"):
            with open(os.path.join(out, name)) as f:
                sources.append(f.read())
    missing = [form for form, mark in JIT_FORMS.items() if not any(mark in s for s in sources)]
    assert not missing, missing
