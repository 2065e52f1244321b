"""The dense adjoint identities of the geometric product on the CPU: tools/proto/adjoint_dense.py against
the Jacobian of the bitmask product, both operands, n = 4..7, 40 random metrics each with negative, scaled and null squares."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dense_adjoint_identities_both_operands():
    sys.path.insert(0, os.path.join(ROOT, "tools", "proto"))
    try:
        import adjoint_dense
    finally:
        sys.path.pop(0)
    assert adjoint_dense.check(n_metrics=40, dims=(4, 5, 6, 7)) <= 1e-12
