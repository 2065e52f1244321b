"""Independent oracle for Clifford products over an arbitrary symmetric bilinear form B (a Gram matrix), in the wedge basis.

It never diagonalises.  Blades E_S = e_s0 ^ e_s1 ^ ... (s0 < s1 < ...) are indexed by bitmask; a multivector is a float array of
length 2^n.  Chevalley's recursion gives every left-multiplication matrix:
    e_i E_S = e_i _| E_S + e_i ^ E_S                     (e_i _| E_S = sum_t (-1)^t B(i, s_t) E_{S - s_t})
    E_S     = e_s0 E_S' - e_s0 _| E_S'                   (S' = S - s0)
so L(E_S) = L(e_s0) L(E_S') - sum_t (-1)^t B(s0, s'_t) L(E_{S' - s'_t}).  O(4^n) per product: n <= 6.
Grade selections per product kind as in the reference (src/ast/expr.rs:180-197).
"""
from __future__ import annotations

import numpy as np

GEOMETRIC, OUTER, INNER, LCONTRACT, RCONTRACT = "gp", "op", "ip", "lc", "rc"


def popcount(m):
    return bin(m).count("1")


def bits_of(m):
    return [i for i in range(m.bit_length()) if (m >> i) & 1]


def blades_of_grade(n, k):
    """component order of grade k: colex rank of the blade = increasing bitmask"""
    return [m for m in range(1 << n) if popcount(m) == k]


def row_blades(n, grades):
    out = []
    for k in sorted(grades):
        out.extend(blades_of_grade(n, k))
    return out


def row_to_mv(n, grades, row):
    v = np.zeros(1 << n)
    v[row_blades(n, grades)] = np.asarray(row, dtype=np.float64)
    return v


def mv_to_row(n, grades, v):
    return np.asarray(v)[row_blades(n, grades)]


def select(kind, k1, k2):
    """grades kept of the product of a k1-vector and a k2-vector (expr.rs:180-197)"""
    if kind == GEOMETRIC:
        return set(range(abs(k1 - k2), k1 + k2 + 1, 2))
    if kind == OUTER:
        return {k1 + k2}
    if kind == INNER:
        return set() if k1 == 0 or k2 == 0 else {abs(k1 - k2)}
    if kind == LCONTRACT:
        return {k2 - k1} if k2 >= k1 else set()
    if kind == RCONTRACT:
        return {k1 - k2} if k1 >= k2 else set()
    raise ValueError(kind)


class GramClifford:
    def __init__(self, gram):
        self.B = np.array(gram, dtype=np.float64)
        self.n = n = self.B.shape[0]
        assert self.B.shape == (n, n) and np.array_equal(self.B, self.B.T)
        self.N = 1 << n
        self.grade = np.array([popcount(m) for m in range(self.N)])
        self._vec = [self._vector_left(i) for i in range(n)]
        self._L = {0: np.eye(self.N)}

    def _vector_left(self, i):
        L = np.zeros((self.N, self.N))
        for S in range(self.N):
            if not (S >> i) & 1:                                   # wedge
                L[S | (1 << i), S] += -1.0 if popcount(S & ((1 << i) - 1)) & 1 else 1.0
            for t, s in enumerate(bits_of(S)):                     # contraction
                L[S ^ (1 << s), S] += (-1.0) ** t * self.B[i, s]
        return L

    def left(self, S):
        """left-multiplication matrix of the blade E_S"""
        if S not in self._L:
            s0 = (S & -S).bit_length() - 1
            Sp = S ^ (1 << s0)
            L = self._vec[s0] @ self.left(Sp)
            for t, s in enumerate(bits_of(Sp)):
                L = L - (-1.0) ** t * self.B[s0, s] * self.left(Sp ^ (1 << s))
            self._L[S] = L
        return self._L[S]

    def gp(self, a, b):
        out = np.zeros(self.N)
        for S in np.nonzero(a)[0]:
            out += a[S] * (self.left(int(S)) @ b)
        return out

    def part(self, a, k):
        return np.where(self.grade == k, a, 0.0)

    def product(self, a, b, kind=GEOMETRIC):
        out = np.zeros(self.N)
        for k1 in range(self.n + 1):
            ak = self.part(a, k1)
            if not ak.any():
                continue
            for k2 in range(self.n + 1):
                bk = self.part(b, k2)
                if not bk.any():
                    continue
                keep = select(kind, k1, k2)
                if keep:
                    p = self.gp(ak, bk)
                    out += np.where(np.isin(self.grade, list(keep)), p, 0.0)
        return out

    def rev(self, a):
        k = self.grade
        return np.where((k * (k - 1) // 2) % 2 == 1, -a, a)

    def ginvol(self, a):
        return np.where(self.grade % 2 == 1, -a, a)

    def g(self, a, k):
        return self.part(a, k)

    def norm_sq(self, a):
        return self.part(self.gp(self.rev(a), a), 0)

    def vinv(self, a):
        return self.rev(a) / self.norm_sq(a)[0]

    def basis_vector(self, i):
        v = np.zeros(self.N)
        v[1 << i] = 1.0
        return v
