// Generation of a Product's component-multiplication list (the slice of the Cayley table it
// needs), in the reference's order T4: (k_left asc, k_right asc, left index asc, right index
// asc), filtered by grade(result) in contribs  (specialize.rs:132-183).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "algebra.hpp"
#include "gaast_hip.h"
#include "grade_set.hpp"

namespace gaast {

// Exact length of the list without generating it: pairs (a,b) with |a|=kl, |b|=kr sharing s
// basis vectors number C(n,kl) C(kl,s) C(n-kl,kr-s) and land in grade kl+kr-2s.
// regressive: C(n,kl) left blades, and a right blade is the left one's complement (n - kl vectors) plus kr - (n - kl) of the left's kl
inline uint64_t comp_mul_count(int n, const std::vector<Contrib>& contribs, bool regressive = false) {
    uint64_t total = 0;
    if (regressive) {
        for (const Contrib& c : contribs) {
            const int g = c.k_left + c.k_right - n;
            if (g < 0 || g > 63 || c.k_left > n || c.k_right > n || !((c.contribs >> g) & 1ULL)) continue;
            total += n_choose_k(n, c.k_left) * n_choose_k(c.k_left, g);
        }
        return total;
    }
    for (const Contrib& c : contribs) {
        for (int s = 0; s <= c.k_left && s <= c.k_right; ++s) {
            int g = c.k_left + c.k_right - 2 * s;
            if (g < 0 || g > 63 || !((c.contribs >> g) & 1ULL)) continue;
            total += n_choose_k(n, c.k_left) * n_choose_k(c.k_left, s) *
                     n_choose_k(n - c.k_left, c.k_right - s);
        }
    }
    return total;
}

// 1 when the right complement of blade s (GAAST_OP_DUAL, gaast_hip.h) carries a minus sign: par(S, ~S); the left complement
// (GAAST_OP_UNDUAL) has par(~S, S) = complement_parity(~S)
inline int complement_parity(int n, uint64_t s) {
    const uint64_t full = n >= 64 ? ~0ULL : ((1ULL << n) - 1ULL);
    return reorder_parity(s & full, ~s & full);
}

// e_a v e_b = undual(dual(e_a) ^ dual(e_b)): non-zero only when a | b is full, then +-e_{a & b}; *neg = the sign
inline bool regressive_blades(int n, uint64_t a, uint64_t b, int* neg) {
    const uint64_t full = n >= 64 ? ~0ULL : ((1ULL << n) - 1ULL);
    if ((a | b) != full) return false;
    const uint64_t ca = ~a & full, cb = ~b & full;   // disjoint: their outer product is +-e_{ca | cb}
    *neg = (complement_parity(n, a) + complement_parity(n, b) + reorder_parity(ca, cb) + complement_parity(n, a & b)) & 1;
    return true;                                      // (undual(e_{ca|cb}) has par(~(ca|cb), ca|cb) = complement_parity(a & b))
}

template <class Emit>
inline void for_each_comp_mul(const BladeTable& bt, const double* metric_diag,
                              const std::vector<Contrib>& contribs, Emit&& emit, bool regressive = false) {
    const int n = bt.n;
    for (const Contrib& c : contribs) {
        if (c.k_left > n || c.k_right > n) continue;  // grade_dim == 0: no blades
        const auto& lb = bt.blade_of[c.k_left];
        const auto& rb = bt.blade_of[c.k_right];
        if (regressive) {  // the same order T4 over the pairs with a | b full; no metric factor
            for (uint32_t li = 0; li < lb.size(); ++li)
                for (uint32_t ri = 0; ri < rb.size(); ++ri) {
                    const uint64_t a = lb[li], b = rb[ri];
                    int neg = 0;
                    if (!regressive_blades(n, a, b, &neg)) continue;
                    const int g = __builtin_popcountll(a & b);
                    if (!((c.contribs >> g) & 1ULL)) continue;
                    emit(gaast_comp_mul{uint32_t(c.k_left), li, uint32_t(c.k_right), ri, uint32_t(g), bt.index_of[a & b], neg ? -1.0 : 1.0});
                }
            continue;
        }
        for (uint32_t li = 0; li < lb.size(); ++li) {
            const uint64_t a = lb[li];
            for (uint32_t ri = 0; ri < rb.size(); ++ri) {
                const uint64_t b = rb[ri];
                const uint64_t r = a ^ b;
                const int g = __builtin_popcountll(r);
                if (!((c.contribs >> g) & 1ULL)) continue;
                gaast_comp_mul m;
                m.left_grade = uint32_t(c.k_left);
                m.left_index = li;
                m.right_grade = uint32_t(c.k_right);
                m.right_index = ri;
                m.result_grade = uint32_t(g);
                m.result_index = bt.index_of[r];
                m.coeff = blades_gp_coeff(n, metric_diag, a, b);
                emit(m);
            }
        }
    }
}

// Adjoint (transposed) list of a product list (l, r -> o, c).  The operand that is differentiated becomes the result and
// the cotangent o takes its place: right = false gives (o, r -> l, c); right = true gives (l, o -> r, c), or (o, l -> r, c)
// with cotangent_first (the operand order of a GAAST_PROD_ADJ_RIGHT node: cotangent, then the other forward operand).
// Forward order is kept, then the entries are ordered stably by result component.
inline std::vector<gaast_comp_mul> transpose_comp_muls(const gaast_comp_mul* fwd, uint64_t n, bool right, bool cotangent_first) {
    std::vector<gaast_comp_mul> out(static_cast<size_t>(n));
    for (uint64_t e = 0; e < n; ++e) {
        const gaast_comp_mul& f = fwd[e];
        gaast_comp_mul& m = out[size_t(e)];
        m.coeff = f.coeff;
        if (!right) {
            m.left_grade = f.result_grade, m.left_index = f.result_index;
            m.right_grade = f.right_grade, m.right_index = f.right_index;
            m.result_grade = f.left_grade, m.result_index = f.left_index;
        } else {
            const uint32_t ag = cotangent_first ? f.result_grade : f.left_grade, ai = cotangent_first ? f.result_index : f.left_index;
            const uint32_t bg = cotangent_first ? f.left_grade : f.result_grade, bi = cotangent_first ? f.left_index : f.result_index;
            m.left_grade = ag, m.left_index = ai;
            m.right_grade = bg, m.right_index = bi;
            m.result_grade = f.right_grade, m.result_index = f.right_index;
        }
    }
    std::stable_sort(out.begin(), out.end(), [](const gaast_comp_mul& a, const gaast_comp_mul& b) {
        return a.result_grade != b.result_grade ? a.result_grade < b.result_grade : a.result_index < b.result_index;
    });
    return out;
}

}  // namespace gaast
