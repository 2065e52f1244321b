// k_gp_mfma32p at n = 12, non-degenerate metric: the quad-plane B image and the address algebra of its step loop.
// ONE statement of the layout for the plan builder (plan_dense.cpp: build_operand_map), the kernel (kernels_dense.hip.hpp: the XOR_STEP
// path) and the host test (tests/cpp/b_planes_driver.cpp).  Plain constexpr functions, no HIP types: the file compiles as
// C++ and as HIP.  (It keeps the .hip.hpp suffix because it decides which bytes the kernel reads: the library's revision
// string hashes device/*.hip.hpp.)
//
// A lane (column c_hi, parity h) multiplies, in step a_hi, the 16 words B[x][2 s2 + h] of block x = a_hi ^ c_hi, in term
// order s2 = s2_of_word(t): four 16-byte quads q = t >> 2.  The block image (mfma32p_b_pos) keeps the quad index inside
// the block's 128 bytes, mixed with a swizzle: the four quads of a lane differ by an XOR, and each needs a live address.
// Here the quad index is the TOP of the position:
//     word position of blade m = (q << 10) | (h << 9) | (x << 2) | e,     x = m >> 5, k = m & 31, h = k & 1,
//                                                                        w = word_of_s2(k >> 1), q = w >> 2, e = w & 3
// so planes are 4 KiB apart, the two h halves of a plane 2 KiB, and block x's quad sits at byte 16 x of its half: quads
// q and q + 1 of one lane are a constant 4,096 bytes apart (an immediate offset of the LDS read), and the 32 lanes of one
// h read 32 distinct blocks of an aligned group of 32 -- 512 contiguous bytes, every 16 lanes of an LDS cycle on 16
// different bank quads -- so no swizzle term is needed.
// The sign stays the address bit above the image (+B at 0, -B at NEG = 4 N bytes).  Quads 0, 1 hold the even-|s2| words
// (|k| parity h), quads 2, 3 the odd ones, and lanes with odd |c_hi| take the odd-|k| quads from the other image: that
// flip is a lane constant, but it differs between the quad pairs, so TWO addresses stay live:
//     xe: quad 0 (quad 1 at +4,096)        xo = xe ^ 8,192 ^ (parity(c_hi) on the NEG bit): quad 2 (quad 3 at +4,096)
// Both move from step a_hi to a_hi + 1 by the same three-operand xor  addr ^ delta(t) ^ (u(a_hi) ^ u(a_hi + 1) on the NEG
// bit), t = the number of trailing ones of a_hi: a_hi -> a_hi + 1 flips the bits P_t = 2^(t+1) - 1, everything in the
// address but u is linear over GF(2) in the bits of a_hi, and u is wave-uniform.
#pragma once

#include <cstdint>

#if defined(__HIP__) || defined(__CUDACC__)
#define GAAST_BP_FN __host__ __device__ inline constexpr
#else
#define GAAST_BP_FN inline constexpr
#endif

namespace gaast {
namespace b_planes {

constexpr int kDim = 12;                              // the only n this layout serves
constexpr uint32_t kImageBytes = 4u << kDim;          // one image; also the byte distance +B -> -B (the NEG address bit)
constexpr uint32_t kNeg = kImageBytes;
constexpr uint32_t kQuadStride = 4096;                // bytes from quad q to quad q + 1 of the same lane and block
constexpr uint32_t kOddQuads = 2 * kQuadStride;       // bytes from quad 0 to quad 2

GAAST_BP_FN uint32_t parity(uint32_t v) {
    v ^= v >> 16;
    v ^= v >> 8;
    v ^= v >> 4;
    v ^= v >> 2;
    v ^= v >> 1;
    return v & 1u;
}

// term t of a step multiplies the words k = 2 s2_of_word(t) + h: even |s2| first (the kernels' mfma16_k)
GAAST_BP_FN uint32_t s2_of_word(uint32_t t) {
    constexpr uint32_t order[16] = {0, 3, 5, 6, 9, 10, 12, 15, 1, 2, 4, 7, 8, 11, 13, 14};
    return order[t & 15u];
}
GAAST_BP_FN uint32_t word_of_s2(uint32_t s2) {
    constexpr uint32_t word[16] = {0, 8, 9, 1, 10, 2, 3, 11, 12, 4, 5, 13, 6, 14, 15, 7};
    return word[s2 & 15u];
}

// position (in words) of blade m of the permuted basis inside one B image
GAAST_BP_FN uint32_t pos(uint32_t m) {
    const uint32_t x = m >> 5, k = m & 31u, h = k & 1u, w = word_of_s2(k >> 1);
    return ((w >> 2) << 10) | (h << 9) | (x << 2) | (w & 3u);
}

// block sign of step a_hi for column c_hi = u(a_hi) ^ parity(c_hi & M(a_hi)); neg_hi: the hi vectors that square to -1.
// M is linear over GF(2) in the bits of a_hi (a suffix parity and an AND), u is quadratic but does not depend on the lane.
GAAST_BP_FN uint32_t suffix_parities(uint32_t a_hi) {   // bit p = parity of the bits of a_hi above p
    uint32_t sp = a_hi >> 1;
    sp ^= sp >> 1;
    sp ^= sp >> 2;
    sp ^= sp >> 4;
    sp ^= sp >> 8;
    return sp;
}
GAAST_BP_FN uint32_t sign_mask(uint32_t a_hi, uint32_t neg_hi) { return suffix_parities(a_hi) ^ (a_hi & neg_hi); }
GAAST_BP_FN uint32_t sign_uniform(uint32_t a_hi, uint32_t neg_hi) {
    return parity(a_hi & suffix_parities(a_hi)) ^ parity(a_hi & neg_hi);
}

// byte offsets inside the item's +B / -B pair at step a_hi = 0 (block sign +)
GAAST_BP_FN uint32_t xe0(uint32_t c_hi, uint32_t h) {
    return (h << 11) | (c_hi << 4) | ((parity(c_hi) & h) ? kNeg : 0u);   // h = 1: quads 0, 1 are the odd-|k| ones
}
GAAST_BP_FN uint32_t xo0(uint32_t c_hi, uint32_t h) { return xe0(c_hi, h) ^ kOddQuads ^ (parity(c_hi) ? kNeg : 0u); }

// lane constant of the move a_hi -> a_hi + 1 for a_hi with t trailing ones (t = 6 also serves 63 -> 64 and 127 -> 0)
GAAST_BP_FN uint32_t delta(int t, uint32_t c_hi, uint32_t neg_hi) {
    const uint32_t P = (2u << t) - 1u;
    return (P << 4) ^ (parity(c_hi & sign_mask(P, neg_hi)) ? kNeg : 0u);
}
// ... and its wave-uniform part, the xor's third operand
GAAST_BP_FN uint32_t delta_uniform(uint32_t a_hi, uint32_t neg_hi) {
    return (sign_uniform(a_hi, neg_hi) ^ sign_uniform(a_hi + 1u, neg_hi)) ? kNeg : 0u;
}

static_assert(word_of_s2(s2_of_word(0)) == 0 && word_of_s2(s2_of_word(5)) == 5 && word_of_s2(s2_of_word(9)) == 9 &&
              word_of_s2(s2_of_word(15)) == 15, "word_of_s2 inverts s2_of_word");
static_assert(pos(0xfffu) < 4096u && pos(0xfffu) != pos(0xffeu), "12-bit positions");

}  // namespace b_planes
}  // namespace gaast
