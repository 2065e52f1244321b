"""Algebras with a diagonal metric, and with a full Gram matrix (reference: src/algebra.rs)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


class MetricAlgebra:
    """`[f64; D]` of the reference (algebra.rs:148-165): the squares of the base vectors."""

    def __init__(self, diag):
        self.diag = [float(x) for x in diag]

    def vec_space_dim(self):                       # algebra.rs:16
        return len(self.diag)

    def grade_dim(self, k):                        # algebra.rs:25-27
        return n_choose_k(len(self.diag), k)

    def base_vec_dot(self, v1, v2):                # algebra.rs:156-165
        return self.diag[v1] if v1 == v2 else 0.0

    def _c_diag(self):
        return (C.c_double * max(1, len(self.diag)))(*self.diag)

    def ortho_basis_blades_gp(self, b1, b2):       # algebra.rs:73-83
        res = C.c_uint64()
        coeff = _lib.lib().gaast_blades_gp(len(self.diag), self._c_diag(), b1, b2, C.byref(res))
        return res.value, coeff

    def component_to_basis_blade(self, grade, index):   # algebra.rs:31-37
        return _lib.lib().gaast_component_to_blade(len(self.diag), grade, index)

    def basis_blade_to_component(self, blade):           # algebra.rs:41-45
        g = C.c_int()
        idx = _lib.lib().gaast_blade_to_component(len(self.diag), blade, C.byref(g))
        return g.value, idx


class OrthoEuclidN(MetricAlgebra):
    """OrthoEuclidN(N) (algebra.rs:173-192): N orthogonal base vectors squaring to 1."""

    def __init__(self, n):
        super().__init__([1.0] * int(n))


class GramAlgebra(MetricAlgebra):
    """A metric given by its full (symmetric) Gram matrix: the reference's `base_vec_dot(v1, v2)` on every pair of base vectors
    (algebra.rs:57-66), e.g. conformal GA in its null basis.  G = Q diag(L) Q^T (gaast_metric_diagonalize): programs are
    specialised for the orthogonal basis f_j = sum_i Q_ij e_i (`.diag` = L, `.basis` = Q) and evaluated on rows in the caller's
    basis, moved into f and back by outermorphisms on the GPU (gaast_hip_program_create_in_basis)."""

    def __init__(self, gram):
        g = np.array(gram, dtype=np.float64)
        if g.ndim != 2 or g.shape[0] != g.shape[1] or not 1 <= g.shape[0] <= 16:
            raise ValueError(f"a Gram matrix is n x n with 1 <= n <= 16, got shape {g.shape}")
        n = g.shape[0]
        g = np.ascontiguousarray(g)
        diag = (C.c_double * n)()
        basis = np.zeros((n, n), dtype=np.float64)
        st = _lib.lib().gaast_metric_diagonalize(n, g.ctypes.data_as(_lib._pd), diag, basis.ctypes.data_as(_lib._pd))
        if st:
            raise _lib.GaastError(st, _lib.lib().gaast_expr_last_error().decode())
        super().__init__(list(diag))
        self.gram = g
        self.basis = basis
        self.gram_is_diagonal = not np.any(g - np.diag(np.diag(g)))

    def base_vec_dot(self, v1, v2):                # algebra.rs:57-66: the Gram matrix
        return float(self.gram[v1][v2])

    def identity_basis(self):
        """True when Q == I exactly: the plain program of MetricAlgebra(diag) runs, bit for bit."""
        return bool(np.array_equal(self.basis, np.eye(self.vec_space_dim())))

    def ortho_basis_blades_gp(self, b1, b2):       # algebra.rs:68-83: restricted to a diagonal Gram matrix
        if not self.gram_is_diagonal:
            raise ValueError("ortho_basis_blades_gp needs a diagonal Gram matrix (the blades of the caller's basis are not orthogonal)")
        return super().ortho_basis_blades_gp(b1, b2)


def as_algebra(alg):
    if isinstance(alg, MetricAlgebra):
        return alg
    if isinstance(alg, int):
        return OrthoEuclidN(alg)
    return MetricAlgebra(alg)


def n_choose_k(n, k):                              # algebra.rs:252-254
    return _lib.lib().gaast_n_choose_k(int(n), int(k))
