"""The plan builder's generated code, pinned byte for byte -- CPU only, no HIP.

tests/cpp/codegen_dump_driver.cpp lowers a fixed corpus with gaast::build_plan and writes every generated artifact of every step:
the hiprtc sources of gaast_jit (slab in registers / slabs in LDS) and gaast_chain, the k_ast_fused micro-op stream, the tables
and settings built next to them, and every table and setting of every product step (the dense kernels' operand maps, result maps and
scales, the lists chained into them, the exact lists), the wiring of every step, every table and setting of the steps the whole-plan
passes build (element-wise pass, reduction with scaling, list chain) and the plan's dead cache buffers.  Length and SHA-256 of each must equal tests/golden/codegen_digests.json (recorded by
tools/record_codegen_digests.py BEFORE a change to the generators).  The runtime compiles these strings and keys its compiled-code
cache by their hash, and uploads these tables as they are: equal bytes are equal kernels on equal operand images."""
import hashlib
import json
import os
import re
import subprocess

import pytest

from helpers import plan_sources

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
    cmd += plan_sources(csrc)
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


def test_corpus_reaches_every_form_of_the_plan_passes(dumped):
    """The steps the whole-plan passes build: the element-wise pass with and without its scaling epilogue, the reduction with
    every scalar operation in both of its kernels' forms, the list chain on either side (the sand*g1 cases chain the LEFT operand
    only: sand9g1_right_first chains the right one) and with an aliased operand; and a cache buffer that a pass marked dead."""
    digests, stdout, out = dumped
    assert {m for m in re.findall(r"EW scale=(\d)", stdout)} == {"0", "1"}
    reduce = re.findall(r"REDUCE op=(\d) wave=(\d+)", stdout)
    assert {r[0] for r in reduce} == {"0", "1", "2"}
    assert {r[1] != "0" for r in reduce} == {True, False}
    links = re.findall(r"LINK side=(\d) alias=(\d)", stdout)
    assert {l[0] for l in links} == {"1", "2"}
    assert any(l[1] != "0" for l in links)
    dead = []
    for name in digests:
        if name.endswith(".plan_node_dead"):
            with open(os.path.join(out, name)) as f:
                dead.append(f.read())
    assert any(" 1" in d.split("node_dead")[1] for d in dead)


def test_corpus_reaches_every_branch_of_the_product_lowering(dumped):
    """Every dense kernel family with every branch of its operand-image and step-field code, the matrix-representation tables, chained
    products and the exact list: the set of (family, branch) pairs the corpus reaches is complete."""
    _, stdout, _ = dumped
    reached = set()
    for line in stdout.splitlines():
        case, name = line.split(" ", 1)[0], line.split(" | ")[0]
        m = re.search(r"DENSE family=(\w+) n=(\d+) full=(\d)(\d) contig=(\d)(\d) scaled=(\d) degenerate=(\d) neg_lo_all=(\d) quads=(\d) chained=(\d) row_scale=(\d)", line)
        if m:
            fam, n = m.group(1), int(m.group(2))
            lfull, rfull, lcontig, rcontig, scaled, degenerate, neg_lo_all, quads, chained, row_scale = (int(x) for x in m.groups()[2:])
            dt = "f64" if "_f64" in case else "f32"
            dealt = lfull and rfull and not lcontig and not rcontig      # the bank-dealing passes run on full operands only
            reached.add((fam, dt))
            if fam in ("MFMA6", "MFMA7") and not chained:
                reached.add((fam, dt, "dealt" if dealt else "row order"))
            if fam == "VECTOR_FMA":
                reached.add((fam, "neg_lo_all" if neg_lo_all else "permuted basis" if "permuted basis" in name else "plain"))
            if fam == "MFMA16X4":
                reached.add((fam, "quad image" if quads else "f64 image"))
                assert quads == (dt == "f32"), line
            if fam in ("MFMA32P", "MFMA32"):
                reached.add((fam, n, "degenerate" if degenerate else "quad planes" if fam == "MFMA32P" and n == 12 else "block image"))
            par = re.search(r"(even|odd) x (even|odd) in Cl\((\d+)\)", name)
            if par and not chained:
                reached.add(("parity", par.group(1), par.group(2)))
                if scaled:
                    reached.add(("parity", "pivot not +-1"))
            if not par and not chained and "adjoint" not in name:
                for tag in ("rescaled basis", "permuted basis"):
                    if tag in name:
                        reached.add(("metric", tag))
                if degenerate:
                    reached.add(("metric", "null vector"))
            adj = re.search(r"adjoint (left|right)", name)
            if adj:
                reached.add(("adjoint", adj.group(1)))
                if degenerate:
                    reached.add(("adjoint", "null vector"))
            if chained:
                assert line.split(" | ")[0].endswith("in LDS"), line
                reached.add(("chained", n + (1 if par else 0), dt))
                if row_scale:
                    reached.add(("chained", "row_scale"))
            if fam == "SPINOR":
                reached.add(("SPINOR", "padded" if case.startswith("spinor7") else "negative vector" if "_neg_" in case else "n = 8"))
        m = re.search(r"LIST beta=(\d) rows=(\d+) empty_rows=(\d+) ell=(\d+)", line)
        if m and case.startswith(("list_", "cfg1_")):
            beta, _, empty_rows, _ = (int(x) for x in m.groups())
            reached.add(("list", "accumulated" if beta else "fresh, empty rows" if empty_rows else "fresh"))
            if "mirrored" in case:
                reached.add(("list", "regressive, mirrored"))
            if case.startswith("list_adj"):
                reached.add(("list", "compact adjoint, exact order"))
    want = {("VECTOR_FMA", "f32"), ("VECTOR_FMA", "f64"), ("VECTOR_FMA", "plain"), ("VECTOR_FMA", "neg_lo_all"), ("VECTOR_FMA", "permuted basis"),
            ("MFMA16X4", "f32"), ("MFMA16X4", "f64"), ("MFMA16X4", "quad image"), ("MFMA16X4", "f64 image"),
            ("MFMA32P", "f32"), ("MFMA32", "f32"), ("MFMA32P", 10, "block image"), ("MFMA32P", 12, "quad planes"), ("MFMA32P", 12, "degenerate"),
            ("MFMA32", 14, "block image"),
            ("metric", "rescaled basis"), ("metric", "permuted basis"), ("metric", "null vector"),
            ("adjoint", "left"), ("adjoint", "right"), ("adjoint", "null vector"),
            ("SPINOR", "f32"), ("SPINOR", "n = 8"), ("SPINOR", "padded"), ("SPINOR", "negative vector"),
            ("chained", "row_scale"),
            ("list", "fresh"), ("list", "fresh, empty rows"), ("list", "accumulated"), ("list", "regressive, mirrored"), ("list", "compact adjoint, exact order"),
            ("parity", "pivot not +-1")}
    want |= {(fam, dt) for fam in ("MFMA6", "MFMA7") for dt in ("f32", "f64")}
    want |= {(fam, dt, how) for fam in ("MFMA6", "MFMA7") for dt in ("f32", "f64") for how in ("dealt", "row order")}
    want |= {("parity", l, r) for l in ("even", "odd") for r in ("even", "odd")}
    want |= {("chained", n, dt) for n in (8, 9) for dt in ("f32", "f64")}
    assert reached == want, (sorted(map(str, want - reached)), sorted(map(str, reached - want)))
