// Non-diagonal metrics (Gram matrices) and changes of basis, host side.
//
//   metric_diagonalize  G = Q diag(L) Q^T with Q orthogonal (cyclic Jacobi in double: no LAPACK, deterministic).  Programs are then
//                       specialised for the orthogonal basis f_j = sum_i Q_ij e_i, whose metric diag(L) the kernels already handle.
//   compound_matrix     the k-th compound C_k(M) of an n x n matrix: the outermorphism of M on grade k, rows and columns in the
//                       library's component order (colex rank of the blade), entry [I][J] = det M[I, J].  Built grade by grade by
//                       Laplace expansion along the first row of each minor, from the (k - 1)-minors.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "algebra.hpp"

namespace gaast {

inline bool gram_is_diagonal(int n, const double* g) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
            if (i != j && g[i * n + j] != 0.0) return false;
    return true;
}

// false: gram not finite / not exactly symmetric / n out of range.  basis[i * n + j] = coordinate i of f_j.
inline bool metric_diagonalize(int n, const double* gram, double* diag, double* basis) {
    if (n < 1 || n > 16 || !gram) return false;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
            if (!std::isfinite(gram[i * n + j]) || gram[i * n + j] != gram[j * n + i]) return false;
    if (gram_is_diagonal(n, gram)) {   // exactly diagonal: Q = I, L = diag(G) bit for bit, original order
        for (int i = 0; i < n; ++i) {
            diag[i] = gram[i * n + i];
            for (int j = 0; j < n; ++j) basis[i * n + j] = i == j ? 1.0 : 0.0;
        }
        return true;
    }
    std::vector<double> a(gram, gram + n * n), v(size_t(n * n), 0.0);
    for (int i = 0; i < n; ++i) v[size_t(i * n + i)] = 1.0;
    auto A = [&](int i, int j) -> double& { return a[size_t(i * n + j)]; };
    for (int sweep = 0; sweep < 100; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) off += std::fabs(A(p, q));
        if (off == 0.0) break;
        for (int p = 0; p < n; ++p) {
            for (int q = p + 1; q < n; ++q) {
                const double apq = A(p, q);
                if (apq == 0.0) continue;
                // after a few sweeps an element below the last bit of both diagonal entries is dropped (it no longer moves them)
                if (sweep > 3 && std::fabs(A(p, p)) + 100.0 * std::fabs(apq) == std::fabs(A(p, p)) &&
                    std::fabs(A(q, q)) + 100.0 * std::fabs(apq) == std::fabs(A(q, q))) {
                    A(p, q) = A(q, p) = 0.0;
                    continue;
                }
                const double theta = (A(q, q) - A(p, p)) / (2.0 * apq);
                double t = 1.0 / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                if (theta < 0.0) t = -t;
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; ++k) {   // A <- J^T A J, J the rotation in the (p, q) plane
                    const double akp = A(k, p), akq = A(k, q);
                    A(k, p) = c * akp - s * akq;
                    A(k, q) = s * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {
                    const double apk = A(p, k), aqk = A(q, k);
                    A(p, k) = c * apk - s * aqk;
                    A(q, k) = s * apk + c * aqk;
                }
                A(p, q) = A(q, p) = 0.0;
                for (int k = 0; k < n; ++k) {
                    double& vkp = v[size_t(k * n + p)];
                    double& vkq = v[size_t(k * n + q)];
                    const double x = vkp, y = vkq;
                    vkp = c * x - s * y;
                    vkq = s * x + c * y;
                }
            }
        }
    }
    double lmax = 0.0;
    for (int i = 0; i < n; ++i) lmax = std::fmax(lmax, std::fabs(A(i, i)));
    const double tiny = 64.0 * 2.220446049250313e-16 * lmax;   // a degenerate metric stays degenerate
    for (int j = 0; j < n; ++j) {
        diag[j] = std::fabs(A(j, j)) <= tiny ? 0.0 : A(j, j);
        int big = 0;   // sign of column j: its largest-magnitude entry (the first of equals) positive
        for (int i = 1; i < n; ++i)
            if (std::fabs(v[size_t(i * n + j)]) > std::fabs(v[size_t(big * n + j)])) big = i;
        const double sg = v[size_t(big * n + j)] < 0.0 ? -1.0 : 1.0;
        for (int i = 0; i < n; ++i) basis[i * n + j] = sg * v[size_t(i * n + j)] + 0.0;
    }
    return true;
}

// C_0 ... C_kmax of m (n x n, row-major): out[k] is C(n,k) x C(n,k), row-major, component order of grade k
// (keep_all = false: only out[kmax] is kept, each lower grade is released once the next one is built)
inline void compound_matrices(int n, const double* m, int kmax, std::vector<std::vector<double>>& out, bool keep_all = true) {
    const BladeTable t(n);
    out.assign(size_t(kmax + 1), {});
    out[0].assign(1, 1.0);
    for (int k = 1; k <= kmax; ++k) {
        const size_t d = t.grade_dim[size_t(k)], dp = t.grade_dim[size_t(k - 1)];
        const std::vector<double>& prev = out[size_t(k - 1)];
        std::vector<double>& cur = out[size_t(k)];
        cur.assign(d * d, 0.0);
        for (size_t I = 0; I < d; ++I) {
            const uint32_t bi = t.blade_of[size_t(k)][I];
            const int i0 = __builtin_ctz(bi);              // first row of the minor
            const size_t Ir = t.index_of[bi & (bi - 1)];   // the other rows: a (k - 1)-minor's row
            for (size_t J = 0; J < d; ++J) {
                uint32_t bj = t.blade_of[size_t(k)][J];
                double acc = 0.0;
                int tpos = 0;
                for (uint32_t rest = bj; rest; rest &= rest - 1, ++tpos) {   // expansion along row i0: column j_t, sign (-1)^t
                    const int jt = __builtin_ctz(rest);
                    const double term = m[i0 * n + jt] * prev[Ir * dp + t.index_of[bj & ~(1u << jt)]];
                    acc += (tpos & 1) ? -term : term;
                }
                cur[I * d + J] = acc;
            }
        }
        if (!keep_all) std::vector<double>().swap(out[size_t(k - 1)]);
    }
}

// Reverse mode of C_k with respect to the matrix: a k x k minor det M[I, J] is linear in each of its entries, with the cofactor
//   d det M[I, J] / d M[i, j] = (-1)^(p_I(i) + p_J(j)) det M[I \ i, J \ j]      (i in I, j in J; p: 0-based position in the ascending blade)
// One term per (I, J, i, j): which entry of W_k = d L / d C_k, which entry of C_{k-1}, the sign and the target (i, j).  The
// order is I, J, i, j ascending (component order of grade k, then positions) -- the host sum and the device table both start here.
struct CompoundVjpTerm {
    uint32_t w;        // I * C(n,k) + J
    uint32_t minor;    // (I \ i) * C(n,k-1) + (J \ j)
    uint16_t target;   // i * n + j
    uint16_t negative; // 1: the cofactor's sign is -1
};

inline void compound_vjp_terms(const BladeTable& t, int k, std::vector<CompoundVjpTerm>& out) {
    out.clear();
    if (k < 1 || k > t.n) return;
    const size_t d = t.grade_dim[size_t(k)], dp = t.grade_dim[size_t(k - 1)];
    out.reserve(d * d * size_t(k) * size_t(k));
    for (size_t I = 0; I < d; ++I) {
        const uint32_t bi = t.blade_of[size_t(k)][I];
        for (size_t J = 0; J < d; ++J) {
            const uint32_t bj = t.blade_of[size_t(k)][J];
            int pi = 0;
            for (uint32_t ri = bi; ri; ri &= ri - 1, ++pi) {
                const int i = __builtin_ctz(ri);
                int pj = 0;
                for (uint32_t rj = bj; rj; rj &= rj - 1, ++pj) {
                    const int j = __builtin_ctz(rj);
                    CompoundVjpTerm e;
                    e.w = uint32_t(I * d + J);
                    e.minor = uint32_t(size_t(t.index_of[bi & ~(1u << i)]) * dp + t.index_of[bj & ~(1u << j)]);
                    e.target = uint16_t(i * t.n + j);
                    e.negative = uint16_t((pi + pj) & 1);
                    out.push_back(e);
                }
            }
        }
    }
}

// dmatrix (n x n, row-major) += grade k's part of d L / d M for W_k = d L / d C_k(M) (C(n,k) x C(n,k), row-major).  Grade 0 adds nothing.
inline void compound_matrix_vjp(int n, int k, const double* m, const double* w, double* dmatrix) {
    if (k < 1) return;
    const BladeTable t(n);
    std::vector<std::vector<double>> c;
    compound_matrices(n, m, k - 1, c, false);
    const std::vector<double>& prev = c[size_t(k - 1)];
    std::vector<CompoundVjpTerm> terms;
    compound_vjp_terms(t, k, terms);
    for (const CompoundVjpTerm& e : terms) {
        const double term = prev[e.minor] * w[e.w];
        dmatrix[e.target] += e.negative ? -term : term;
    }
}

// determinant by Gaussian elimination with partial pivoting (m: n x n, row-major)
inline double matrix_determinant(int n, const double* m) {
    std::vector<double> a(m, m + size_t(n) * size_t(n));
    double det = 1.0;
    for (int c = 0; c < n; ++c) {
        int piv = c;
        for (int r = c + 1; r < n; ++r)
            if (std::fabs(a[size_t(r * n + c)]) > std::fabs(a[size_t(piv * n + c)])) piv = r;
        if (a[size_t(piv * n + c)] == 0.0) return 0.0;
        if (piv != c) {
            for (int k = 0; k < n; ++k) std::swap(a[size_t(piv * n + k)], a[size_t(c * n + k)]);
            det = -det;
        }
        det *= a[size_t(c * n + c)];
        for (int r = c + 1; r < n; ++r) {
            const double f = a[size_t(r * n + c)] / a[size_t(c * n + c)];
            for (int k = c; k < n; ++k) a[size_t(r * n + k)] -= f * a[size_t(c * n + k)];
        }
    }
    return det;
}

// does the orthogonal basis Q of a Gram metric reverse the orientation (det Q = -1)?  The complement in the caller's basis is
// det(Q) times the complement in the orthogonal basis (gaast_hip.h: GAAST_OP_DUAL): such a program is lowered with Plan::mirrored
inline bool basis_is_mirrored(int n, const double* q) { return matrix_determinant(n, q) < 0.0; }

}  // namespace gaast
