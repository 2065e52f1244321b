// The operand images of the dense-product kernels, stated once: the order in which a kernel multiplies the words of a block (its
// term-order table), where the staging puts blade m of the permuted basis inside an image (its position function), how many low
// basis vectors a family folds into compile-time signs, how k_gp_mfma6 deals components to lanes, and what a workgroup of each
// family holds in LDS.  The plan builder (plan_dense.cpp: build_operand_map; plan_passes.cpp: chain_sparse_into_dense), the kernels
// (kernels_dense.hip.hpp take their term orders from here), the launcher (runtime.hip: prepare_dense) and a host test
// (tests/cpp/dense_images_driver.cpp) read this file.  Plain constexpr functions, no HIP types: it compiles as C++ and as HIP.
// (The .hip.hpp suffix puts it into the library's revision string, which hashes device/*.hip.hpp.)
// The quad-plane B image of k_gp_mfma32p at n = 12 has a header of its own, included here: b_planes::pos.
#pragma once

#include <cstddef>
#include <cstdint>

#include "mfma32p_b_planes.hip.hpp"

#ifndef GAAST_MFMA6_WAVES
#define GAAST_MFMA6_WAVES 1   /* (build switch for A/B runs) independent waves per workgroup of k_gp_mfma6 */
#endif

namespace gaast {

// which kernel family runs a PRODUCT_DENSE step
enum class DenseFamily {
    VECTOR_FMA,  // k_gp_dense<T>
    MFMA6,       // k_gp_mfma6<T> (n = 6: four 16x16x4 instructions per item, the two top vectors split over the tile's rows and columns)
    MFMA7,       // k_gp_mfma7<T> (n = 7: lo = 3 bits, the top vector split over the two sides of the 16 x 16 tile)
    MFMA16X4,    // k_gp_mfma16x4<T> (lo = 4 bits, one item per workgroup): f64 n = 8 ... 12, f32 n = 8, 9
    MFMA32,      // k_gp_mfma32 (f32, n = 14)
    MFMA32P,     // k_gp_mfma32p (image-pair form, f32, n = 10 ... 13)
    SPINOR       // opt-in matrix-representation kernels (GAAST_FLAG_SPINOR_GEMM)
};

namespace dense_images {

// ---- term orders: which word k of a B block (the b_lo part of the blade) an instruction multiplies ----
// k_gp_mfma32p / k_gp_mfma32: term t of a step multiplies the words k = 2 mfma16_k(t) + h, even |k >> 1| first.  The table is
// b_planes::s2_of_word (its inverse: b_planes::word_of_s2); k_gp_mfma32 takes its terms in plain order, s2 = t.
GAAST_BP_FN int mfma16_k(int t) { return int(b_planes::s2_of_word(uint32_t(t))); }
// k_gp_mfma16x4<double>: lane group kq multiplies k = 4 s + kq in instruction s
GAAST_BP_FN int mfma16d_k(int kq, int s) { return 4 * s + kq; }
// k_gp_mfma16x4<float>: the four words of a lane group are ONE 16-byte quad and have one |k| parity (groups 0, 1 even, 2, 3 odd)
GAAST_BP_FN int mfma16q_k(int kq, int s) {
    constexpr int tab[4][4] = {{0, 3, 5, 6}, {9, 10, 12, 15}, {1, 2, 4, 7}, {8, 11, 13, 14}};
    return tab[kq][s];
}
// k_gp_mfma7: a lane group's two words of a step, one |k| parity
GAAST_BP_FN int mfma7_k(int kq, int s) {
    constexpr int tab[4][2] = {{0, 3}, {5, 6}, {1, 2}, {4, 7}};
    return tab[kq][s];
}
// the inverses the host needs: the (kq, s) that multiplies word k, found in the tables above (-1: none, which no k has)
GAAST_BP_FN int mfma16q_kq(int k) {
    for (int kq = 0; kq < 4; ++kq)
        for (int s = 0; s < 4; ++s)
            if (mfma16q_k(kq, s) == k) return kq;
    return -1;
}
GAAST_BP_FN int mfma16q_s(int k) {
    for (int kq = 0; kq < 4; ++kq)
        for (int s = 0; s < 4; ++s)
            if (mfma16q_k(kq, s) == k) return s;
    return -1;
}
GAAST_BP_FN int mfma7_kq(int k) {
    for (int kq = 0; kq < 4; ++kq)
        for (int s = 0; s < 2; ++s)
            if (mfma7_k(kq, s) == k) return kq;
    return -1;
}
GAAST_BP_FN int mfma7_s(int k) {
    for (int kq = 0; kq < 4; ++kq)
        for (int s = 0; s < 2; ++s)
            if (mfma7_k(kq, s) == k) return s;
    return -1;
}

// ---- positions (in elements) of blade m of the permuted basis inside one operand image ----
// k_gp_dense, both operands: blocks of 16, the four 16-byte quads of block x rotated by (x >> 2) & 3 so that 16 lanes reading the
// same logical quad of 16 different blocks touch 16 different bank quads
GAAST_BP_FN uint32_t vec_pos(uint32_t m) {
    const uint32_t x = m >> 4, lo = m & 15u;
    return (x << 4) | ((((lo >> 2) ^ (x >> 2)) & 3u) << 2) | (lo & 3u);
}
// k_gp_mfma32's B image: block x = m >> 5; inside it the components are de-interleaved by the parity of k = m & 31 (even k first),
// 8 quads rotated by (x >> 1) & 7
GAAST_BP_FN uint32_t mfma32_b_pos(uint32_t m) {
    const uint32_t x = m >> 5, k = m & 31u;
    const uint32_t lq = ((k & 1u) << 2) | (k >> 3);   // logical quad: parity * 4 + (k / 2) / 4
    return (x << 5) | (((lq ^ (x >> 1)) & 7u) << 2) | ((k >> 1) & 3u);
}
// k_gp_mfma32p's block B image: the lane's 16 words (k of one parity) in term order -- even |k >> 1| first --, quads rotated as in
// mfma32_b_pos.  (n = 12 with no null vector among the hi vectors -- the instantiations <false, 12, *, *>, whose step loop keeps
// live B addresses: the quad-plane image, b_planes::pos, instead)
GAAST_BP_FN uint32_t mfma32p_b_pos(uint32_t m) {
    const uint32_t x = m >> 5, k = m & 31u, w = b_planes::word_of_s2(k >> 1);
    const uint32_t lq = ((k & 1u) << 2) | (w >> 2);
    return (x << 5) | (((lq ^ (x >> 1)) & 7u) << 2) | (w & 3u);
}
// k_gp_mfma16x4<double>'s B image: word k of block x at k ^ (((x >> 1) & 7) << 1)
GAAST_BP_FN uint32_t mfma16d_b_pos(uint32_t m) {
    const uint32_t x = m >> 4, k = m & 15u;
    return (x << 4) | (k ^ (((x >> 1) & 7u) << 1));
}
// k_gp_mfma16x4<float>'s B image: word k = mfma16q_k(kq, s) of block x in quad kq ^ (((x >> 2) & 1) << 1), slot s
GAAST_BP_FN uint32_t mfma16q_b_pos(uint32_t m) {
    const uint32_t x = m >> 4, k = m & 15u;
    return (x << 4) | ((uint32_t(mfma16q_kq(int(k))) ^ (((x >> 2) & 1u) << 1)) << 2) | uint32_t(mfma16q_s(int(k)));
}
// k_gp_mfma7, blade = (top, hi3, lo3).  A image: u * 72 + (a_hi3, a_lo) -- 128 blades in [0, 136), the eight elements after each
// half unused; B image: [kq][v][b_hi3][s] with k = mfma7_k(kq, s)
constexpr uint32_t kMfma7ASpan = 136;
GAAST_BP_FN uint32_t mfma7_a_pos(uint32_t m) { return (m & 63u) + (m >> 6) * 72u; }
GAAST_BP_FN uint32_t mfma7_b_pos(uint32_t m) {
    const uint32_t v = m >> 6, bh = (m >> 3) & 7u, k = m & 7u;
    return ((uint32_t(mfma7_kq(int(k))) * 16u + v * 8u + bh) << 1) | uint32_t(mfma7_s(int(k)));
}
// (the A images of k_gp_mfma16x4, k_gp_mfma32 and k_gp_mfma32p are in blade order; k_gp_mfma6 derives its image slots from the
//  blade itself: position = blade)

// ---- the blade split: the low basis vectors whose signs are lane constants (neg_lo); the rest are steps (neg_hi, zero_hi) ----
GAAST_BP_FN int lo_bits(DenseFamily fam) {
    return (fam == DenseFamily::MFMA32 || fam == DenseFamily::MFMA32P) ? 5 : fam == DenseFamily::MFMA7 ? 3 : fam == DenseFamily::MFMA6 ? 0 : 4;
}
// image-pair kernels: the b_hi part of (-1)^(|a_hi| |b_lo|), |a_hi| = |b_hi| + |c_hi| (mod 2), lives in the B image (the kernel
// supplies the c_hi part): 1 = blade m of the B image is stored negated.  k_gp_mfma7 folds the hi3 part only -- the top vector's
// share is in the kernel's A and result signs
GAAST_BP_FN uint32_t b_image_sign(DenseFamily fam, uint32_t m) {
    const int L = lo_bits(fam);
    const uint32_t hi = fam == DenseFamily::MFMA7 ? (m >> 3) & 7u : m >> L, lo = m & ((1u << L) - 1u);
    const bool folds = fam == DenseFamily::MFMA16X4 || fam == DenseFamily::MFMA32P || fam == DenseFamily::MFMA7;
    return folds ? (b_planes::parity(hi) & b_planes::parity(lo)) : 0u;
}

// ---- k_gp_mfma6: lane q moves the component of map entry q into its four image slots.  Entries are dealt to lanes so that the
// lanes sharing an LDS cycle of a store hit different banks (row order: 73 % of the LDS cycles were conflicts,
// profiles/r04_gp6f32_pmc_first_version.csv).  blade = (top2 | hi2 | lo2) = (u, ah, al) / (v, bh, bl):
//   f32 (32 lanes per cycle): A: bank = 16 (al ^ kq)_0 + 4 u + ah    -> group = al_1;       B (slot order
//        rotated by bl in the kernel): bank = 16 (bh ^ s)_0 + 4 v + s -> group = bh_1
//   f64 (16 lanes per cycle, 8-byte units mod 16): A: (u_0, al ^ kq, ah_0) -> group = (u_1, ah_1);  B: (v, bh_0, bl_0)
//        -> group = (bh_1, bl_1)
GAAST_BP_FN uint32_t mfma6_lane_of(uint32_t blade, bool right, bool f32) {
    const uint32_t t = blade >> 4, h = (blade >> 2) & 3u, l = blade & 3u;
    if (!right) return f32 ? ((l >> 1) << 5) | ((l & 1u) << 4) | (t << 2) | h
                           : ((((t >> 1) << 1) | (h >> 1)) << 4) | ((t & 1u) << 3) | (l << 1) | (h & 1u);
    return f32 ? ((h >> 1) << 5) | ((h & 1u) << 4) | (t << 2) | l
               : ((((h >> 1) << 1) | (l >> 1)) << 4) | (t << 2) | ((h & 1u) << 1) | (l & 1u);
}

// ---- what a workgroup of a family is and holds: threads, items staged at once, 2^n-element operand images per item (+A, -A,
// +B, -B, or A and B; k_gp_mfma6: 64-element slot planes), and the bytes of LDS all of that takes with the kernel's padding and
// zero words.  (elem: 4 or 8.  f64 has no k_gp_mfma32*: such a step would run on k_gp_dense, and is sized so.)
struct Geometry {
    int threads, items, images;
    size_t bytes;
};
GAAST_BP_FN Geometry geometry(DenseFamily fam, int n, int elem) {
    const size_t N = size_t(1) << n, e = size_t(elem);
    switch (fam) {
    case DenseFamily::MFMA32:
    case DenseFamily::MFMA32P:
        if (elem == 4) {
            const int wpi = 1 << (n - 10);   // waves per item
            const int threads = wpi > 4 ? wpi * 64 : 256, items = (threads / 64) / wpi;
            if (fam == DenseFamily::MFMA32P) return {threads, items, 4, (size_t(items) * 4 * N + 16) * e};   // + 16 zeros
            return {threads, items, 2, size_t(items) * 2 * N * e};
        }
        break;
    case DenseFamily::MFMA16X4: return {64 << (n - 8), 1, 4, (4 * N + 32) * e};   // +B, -B, +A, 16 spare, -A images, 16 zeros
    case DenseFamily::MFMA7: return {64, 1, 4, 560 * e};                          // +B, -B, +A (u = 1 half 72 further), -A 144 further, 16 zeros
    case DenseFamily::MFMA6:                                                      // + a dummy element per lane (stores of vanishing slots)
        return {64 * GAAST_MFMA6_WAVES, GAAST_MFMA6_WAVES, 8, (size_t(elem == 8 ? 4096 : 2048) + 64 * e) * GAAST_MFMA6_WAVES};
    default: break;
    }
    const int lpi = 1 << (n - 4);   // k_gp_dense: a lane per 16 result components
    const int threads = lpi > 256 ? lpi : 256, items = threads / lpi;
    return {threads, items, 2, size_t(items) * (2 * N + (items > 1 ? 4 : 0)) * e};
}

// every entry of every table, so that a slip in one is a build error: the inverses invert, each word of a block has one term
GAAST_BP_FN bool tables_consistent() {
    for (int t = 0; t < 16; ++t)
        if (b_planes::word_of_s2(uint32_t(mfma16_k(t))) != uint32_t(t) || b_planes::s2_of_word(b_planes::word_of_s2(uint32_t(t))) != uint32_t(t)) return false;
    for (int k = 0; k < 16; ++k)
        if (mfma16q_kq(k) < 0 || mfma16q_k(mfma16q_kq(k), mfma16q_s(k)) != k || mfma16d_k(k & 3, k >> 2) != k) return false;
    for (int k = 0; k < 8; ++k)
        if (mfma7_kq(k) < 0 || mfma7_k(mfma7_kq(k), mfma7_s(k)) != k) return false;
    for (int kq = 0; kq < 4; ++kq)   // one |k| parity per lane group: its words come from one image
        for (int s = 0; s < 4; ++s)
            if (b_planes::parity(uint32_t(mfma16q_k(kq, s))) != uint32_t(kq >> 1) || b_planes::parity(uint32_t(mfma7_k(kq, s & 1))) != uint32_t(kq >> 1)) return false;
    return true;
}
static_assert(tables_consistent(), "a term-order table and its inverse disagree");

}  // namespace dense_images
}  // namespace gaast
