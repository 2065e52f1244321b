#!/usr/bin/env python3
"""Record tests/golden/codegen_digests.json: length and SHA-256 of every artifact tests/test_codegen_digests.py pins.

Run it on the commit whose generated code is to be kept -- BEFORE a change to the plan's code generators, never after: a
fixture recorded from the code under test pins nothing.  CPU only (g++).  A second argument names another checkout's
gaast_amd/csrc to build the driver against.

    python3 tools/record_codegen_digests.py [output.json [csrc]]
"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_codegen_digests as t            # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN
    csrc = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "gaast_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        digests, stdout = t.build_and_run(csrc, os.path.join(tmp, "out"), os.path.join(tmp, "codegen_dump"))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(digests, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(digests), "artifacts of", len(stdout.splitlines()), "steps ->", out)


if __name__ == "__main__":
    main()
