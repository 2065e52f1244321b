// The operand images of the dense-product kernels (gaast_amd/csrc/device/dense_images.hip.hpp), checked on the CPU under
// AddressSanitizer + UBSan, the header alone:
//   1. every position function is a bijection from the blades of its image onto [0, image size) (k_gp_mfma7's A image: into the
//      136 elements it documents, the eight after each half unused); k_gp_mfma6's dealing is a permutation of the 64 lanes;
//   2. each inverse table inverts its term-order table over all entries;
//   3. lo_bits and the workgroup geometry agree with the image sizes;
//   4. for each family, the word a kernel lane reads for (step, term) -- the address arithmetic of kernels_dense.hip.hpp, restated
//      here per kernel -- is the word the position function placed there, through the shared term-order tables.
// (The quad-plane image of k_gp_mfma32p at n = 12 has tests/cpp/b_planes_driver.cpp.)
// Build: g++ -std=c++17 -fsanitize=address,undefined -I gaast_amd/csrc/device tests/cpp/dense_images_driver.cpp
#include <cstdio>
#include <vector>

#include "dense_images.hip.hpp"

namespace di = gaast::dense_images;
using gaast::DenseFamily;

static int failures = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            if (failures < 20) std::printf("CHECK failed: %s (line %d)\n", #c, __LINE__); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static uint32_t par(uint32_t v) { return uint32_t(__builtin_popcount(v)) & 1u; }

// pos maps [0, 2^n) one-to-one into [0, span); with span == 2^n: onto
template <typename F>
static std::vector<int> injective(F pos, int n, uint32_t span) {
    std::vector<int> inv(span, -1);
    for (uint32_t m = 0; m < (1u << n); ++m) {
        const uint32_t p = pos(m);
        CHECK(p < span);
        if (p >= span) continue;
        CHECK(inv[p] < 0);
        inv[p] = int(m);
    }
    return inv;
}

static void bijections() {
    for (int n = 8; n <= 13; ++n) injective(di::vec_pos, n, 1u << n);
    for (int n = 10; n <= 14; ++n) injective(di::mfma32_b_pos, n, 1u << n);
    for (int n = 10; n <= 13; ++n) injective(di::mfma32p_b_pos, n, 1u << n);
    for (int n = 8; n <= 12; ++n) injective(di::mfma16d_b_pos, n, 1u << n);
    for (int n = 8; n <= 9; ++n) injective(di::mfma16q_b_pos, n, 1u << n);
    injective(gaast::b_planes::pos, gaast::b_planes::kDim, 1u << gaast::b_planes::kDim);
    injective(di::mfma7_b_pos, 7, 128);
    const std::vector<int> a7 = injective(di::mfma7_a_pos, 7, di::kMfma7ASpan);
    for (uint32_t p = 0; p < di::kMfma7ASpan; ++p) CHECK((a7[p] < 0) == ((p >= 64 && p < 72) || p >= 136));
    for (int right = 0; right < 2; ++right)
        for (int f32 = 0; f32 < 2; ++f32) injective([&](uint32_t b) { return di::mfma6_lane_of(b, right != 0, f32 != 0); }, 6, 64);
    std::printf("%s  bijections\n", failures ? "FAILED" : "ok");
}

static void inverse_tables() {
    CHECK(di::tables_consistent());
    uint32_t seen16 = 0, seen16q = 0, seen16d = 0, seen7 = 0;
    for (int t = 0; t < 16; ++t) {
        seen16 |= 1u << di::mfma16_k(t);
        CHECK(gaast::b_planes::word_of_s2(uint32_t(di::mfma16_k(t))) == uint32_t(t));
    }
    for (int kq = 0; kq < 4; ++kq)
        for (int s = 0; s < 4; ++s) {
            const int k = di::mfma16q_k(kq, s), kd = di::mfma16d_k(kq, s);
            seen16q |= 1u << k;
            seen16d |= 1u << kd;
            CHECK(di::mfma16q_kq(k) == kq && di::mfma16q_s(k) == s);
            if (s < 2) {
                const int k7 = di::mfma7_k(kq, s);
                seen7 |= 1u << k7;
                CHECK(di::mfma7_kq(k7) == kq && di::mfma7_s(k7) == s);
            }
        }
    CHECK(seen16 == 0xffffu && seen16q == 0xffffu && seen16d == 0xffffu && seen7 == 0xffu);
    CHECK(di::mfma16q_kq(16) < 0 && di::mfma7_kq(8) < 0);
    std::printf("%s  inverse tables\n", failures ? "FAILED" : "ok");
}

static void geometry_and_split() {
    struct Case { DenseFamily fam; int n_lo, n_hi, elem; };
    const Case cases[] = {{DenseFamily::VECTOR_FMA, 6, 13, 4}, {DenseFamily::VECTOR_FMA, 6, 13, 8}, {DenseFamily::MFMA6, 6, 6, 4}, {DenseFamily::MFMA6, 6, 6, 8},
                          {DenseFamily::MFMA7, 7, 7, 4},       {DenseFamily::MFMA7, 7, 7, 8},       {DenseFamily::MFMA16X4, 8, 9, 4}, {DenseFamily::MFMA16X4, 8, 12, 8},
                          {DenseFamily::MFMA32P, 10, 13, 4},   {DenseFamily::MFMA32, 14, 14, 4}};
    for (const Case& c : cases)
        for (int n = c.n_lo; n <= c.n_hi; ++n) {
            const di::Geometry g = di::geometry(c.fam, n, c.elem);
            const size_t N = size_t(1) << n, images = size_t(g.items) * size_t(g.images) * (c.fam == DenseFamily::MFMA6 ? 64 : N) * size_t(c.elem);
            CHECK(g.threads >= 64 && g.threads <= 1024 && g.threads % 64 == 0 && g.items >= 1);
            CHECK(g.bytes >= images && g.bytes <= images + size_t(g.items) * 32 + 512);   // the images, and at most a few padding and zero words
            CHECK(g.bytes <= 160 * 1024);
            const int L = di::lo_bits(c.fam), waves = g.threads / 64;
            switch (c.fam) {
            case DenseFamily::VECTOR_FMA: CHECK(L == 4 && g.threads == g.items << (n - L)); break;           // a lane per block of 2^lo components
            case DenseFamily::MFMA16X4: CHECK(L == 4 && g.items == 1 && waves * 16 == 1 << (n - L)); break;   // a wave per 16 result columns
            case DenseFamily::MFMA32:
            case DenseFamily::MFMA32P: CHECK(L == 5 && waves * 32 == g.items << (n - L)); break;              // a wave per 32 result columns
            case DenseFamily::MFMA7: CHECK(L == 3 && waves == 1 && g.items == 1 && g.bytes == 560u * size_t(c.elem)); break;
            default: CHECK(L == 0 && waves == g.items); break;                                                // k_gp_mfma6: a wave per item
            }
        }
    // f64 has no k_gp_mfma32*: sized as k_gp_dense
    CHECK(di::geometry(DenseFamily::MFMA32P, 10, 8).bytes == di::geometry(DenseFamily::VECTOR_FMA, 10, 8).bytes);
    // k_gp_mfma7 (elements): +B, -B in [0, 256), +A at 256, -A 144 further, 16 zeros at 544
    CHECK(di::kMfma7ASpan <= 144 && 256 + 144 + di::kMfma7ASpan <= 544 && 544 + 16 == 560);
    // the quad-plane image is one of k_gp_mfma32p's four: +16 zero words
    CHECK(di::geometry(DenseFamily::MFMA32P, gaast::b_planes::kDim, 4).bytes == 4u * gaast::b_planes::kImageBytes + 64u);
    // the B image folds (-1)^(|b_hi| |b_lo|) over the family's split (k_gp_mfma7: the hi3 part)
    for (uint32_t m = 0; m < 4096; ++m) {
        CHECK(di::b_image_sign(DenseFamily::MFMA16X4, m) == (par(m >> 4) & par(m & 15u)));
        CHECK(di::b_image_sign(DenseFamily::MFMA32P, m) == (par(m >> 5) & par(m & 31u)));
        CHECK(di::b_image_sign(DenseFamily::MFMA7, m & 127u) == (par((m >> 3) & 7u) & par(m & 7u)));
        CHECK(di::b_image_sign(DenseFamily::MFMA32, m) == 0 && di::b_image_sign(DenseFamily::VECTOR_FMA, m) == 0 && di::b_image_sign(DenseFamily::MFMA6, m & 63u) == 0);
    }
    std::printf("%s  geometry and blade split\n", failures ? "FAILED" : "ok");
}

// what each kernel's lanes read, restated from its address arithmetic
static void lane_reads() {
    // k_gp_dense (BlockStep::step): logical quad q of block x is read at quad q ^ ((x >> 2) & 3); its element e is component 4 q + e
    for (uint32_t x = 0; x < 512; ++x)
        for (uint32_t q = 0; q < 4; ++q)
            for (uint32_t e = 0; e < 4; ++e) CHECK(di::vec_pos((x << 4) | (4 * q + e)) == ((x << 4) | ((q ^ ((x >> 2) & 3u)) << 2) | e));
    // k_gp_mfma32 / k_gp_mfma32p (block image), lane (c_hi, h), step a_hi: quad q at bq[q] ^ sx; word t = 4 q + e of the lane is
    // term t: k = 2 t + h (k_gp_mfma32), k = 2 mfma16_k(t) + h (k_gp_mfma32p, whose odd-|c_hi| lanes take the quads with (q >> 1) ^ h
    // from the -B image: the quads of odd |k|)
    for (uint32_t c_hi = 0; c_hi < 512; c_hi += 3)
        for (uint32_t a_hi = 0; a_hi < 512; a_hi += 5)
            for (uint32_t h = 0; h < 2; ++h)
                for (uint32_t q = 0; q < 4; ++q) {
                    const uint32_t bq = (c_hi << 7) | (((((h << 2) | q) ^ (c_hi >> 1)) & 7u) << 4);
                    const uint32_t sx = (a_hi << 7) | (((a_hi >> 1) & 7u) << 4);
                    for (uint32_t e = 0; e < 4; ++e) {
                        const uint32_t word = ((bq ^ sx) >> 2) + e, t = 4 * q + e, x = a_hi ^ c_hi;
                        CHECK(di::mfma32_b_pos((x << 5) | (2 * t + h)) == word);
                        const uint32_t k = 2u * uint32_t(di::mfma16_k(int(t))) + h;
                        CHECK(di::mfma32p_b_pos((x << 5) | k) == word);
                        CHECK(par(k) == (((q >> 1) ^ h) & 1u));
                    }
                }
    // k_gp_mfma16x4, lane (c_hi, kq), step a_hi, instruction s: bk[s] ^ sx
    for (uint32_t c_hi = 0; c_hi < 256; ++c_hi)
        for (uint32_t a_hi = 0; a_hi < 256; a_hi += 3)
            for (uint32_t kq = 0; kq < 4; ++kq) {
                const uint32_t x = a_hi ^ c_hi;
                // f32 (16-byte blocks of 4 words: BS = 6): the lane's quad, words s = 0 ... 3 of it
                const uint32_t bkq = (c_hi << 6) | ((kq ^ (((c_hi >> 2) & 1u) << 1)) << 4), sxq = (a_hi << 6) | ((((a_hi >> 2) & 1u) << 1) << 4);
                for (uint32_t s = 0; s < 4; ++s) {
                    const uint32_t k = uint32_t(di::mfma16q_k(int(kq), int(s)));
                    CHECK(di::mfma16q_b_pos((x << 4) | k) == ((bkq ^ sxq) >> 2) + s);
                    CHECK(par(k) == (kq >> 1));   // odd-|c_hi| lanes take the words of groups kq >= 2 from the -B image
                    // f64 (BS = 7, ES = 3): one word per instruction
                    const uint32_t kd = uint32_t(di::mfma16d_k(int(kq), int(s)));
                    const uint32_t bkd = (c_hi << 7) | ((((c_hi >> 1) & 7u) << 4) ^ (kd << 3)), sxd = (a_hi << 7) | (((a_hi >> 1) & 7u) << 4);
                    CHECK(di::mfma16d_b_pos((x << 4) | kd) == (bkd ^ sxd) >> 3);
                }
            }
    // k_gp_mfma7, lane (hi, lo3, kq): B pair of step a_hi3 at pair index kq * 16 + v * 8 + b_hi3 (v = hi, b_hi3 = lo3 ^ a_hi3), its two
    // words are the terms s = 0, 1; A operand of instruction s at u * 72 + a_hi3 * 8 + a_lo (u = hi, a_lo = lo3 ^ k)
    for (uint32_t hi = 0; hi < 2; ++hi)
        for (uint32_t lo3 = 0; lo3 < 8; ++lo3)
            for (uint32_t kq = 0; kq < 4; ++kq)
                for (uint32_t ah = 0; ah < 8; ++ah)
                    for (uint32_t s = 0; s < 2; ++s) {
                        const uint32_t k = uint32_t(di::mfma7_k(int(kq), int(s))), bh = lo3 ^ ah, al = lo3 ^ k;
                        CHECK(di::mfma7_b_pos((hi << 6) | (bh << 3) | k) == ((kq * 16 + hi * 8 + bh) << 1) + s);
                        CHECK(di::mfma7_a_pos((hi << 6) | (ah << 3) | al) == hi * 72 + ah * 8 + al);
                        CHECK(par(k) == par(uint32_t(di::mfma7_k(int(kq), 0))));   // both words of a pair come from one image
                    }
    std::printf("%s  lane reads\n", failures ? "FAILED" : "ok");
}

int main() {
    bijections();
    inverse_tables();
    geometry_and_split();
    lane_reads();
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
