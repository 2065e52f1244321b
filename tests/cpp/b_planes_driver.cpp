// The quad-plane B image of k_gp_mfma32p<false, 12, *, *> (gaast_amd/csrc/device/mfma32p_b_planes.hip.hpp), checked on the
// CPU under AddressSanitizer + UBSan.  Two parts:
//   1. the header alone: the position function is a bijection on 0 ... 4095, and for every lane (c_hi, h) the two live
//      addresses, started at xe0 / xo0 and moved by delta(t) ^ delta_uniform(a_hi) as the kernel's step loop moves them,
//      hold in every step a_hi the 16 words B[a_hi ^ c_hi][2 s2 + h] in term order, from the image whose sign is
//          (block sign of (a_hi, c_hi), counted here from the definition: inversions of the hi vectors and their squares)
//          ^ (|c_hi| |k| mod 2: the part of (-1)^(|a_hi| |k|) that the host map does not fold into the image),
//      never leave the item's +B / -B pair, and are back at their start after 128 steps (a persistent workgroup's next
//      item); the 16 lanes that share an LDS cycle of a ds_read_b128 read 16 different bank quads -- for 16 consecutive
//      lanes, 256 contiguous, aligned bytes once the sign bit is set aside (lanes of different block signs read different
//      images, 16 KiB = 64 x 256 bytes apart: the same banks).
//   2. with the plan builder: the right operand's map of a full x full product at n = 12 in f32 uses that position function
//      exactly when the launcher picks the non-degenerate instantiation, and the images staged from the maps, read by the
//      address walk and multiplied as the kernel multiplies them, give the product the plain sign formula gives.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gaast_expr.h"
#include "mfma32p_b_planes.hip.hpp"
#include "plan.hpp"

namespace bp = gaast::b_planes;

static int failures = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            if (failures < 20) std::printf("CHECK failed: %s (line %d)\n", #c, __LINE__); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static uint32_t popc(uint32_t v) { return uint32_t(__builtin_popcount(v)); }

// sign of e_A e_B restricted to the hi vectors, from the definition: inversions, and the vectors of A & B that square to -1
static uint32_t block_sign_by_definition(uint32_t a_hi, uint32_t b_hi, uint32_t neg_hi) {
    uint32_t par = 0;
    for (int p = 1; p < 7; ++p)
        if ((a_hi >> p) & 1u) par ^= popc(b_hi & ((1u << p) - 1u)) & 1u;
    return par ^ (popc(a_hi & b_hi & neg_hi) & 1u);
}

static int step_pattern(uint32_t a_hi) {   // the kernel's choice of delta register: trailing ones of the step inside its chunk of 64
    const uint32_t j = a_hi & 63u;
    return j < 63u ? __builtin_ctz(~j) : 6;
}

// the lanes that share one LDS cycle of a ds_read_b128 (four groups of 16 per wave)
static const int kCycleGroups[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                        {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                        {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                        {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};

static void header_invariants(uint32_t neg_hi, const char* what) {
    std::vector<int> inv(4096, -1);
    for (uint32_t m = 0; m < 4096; ++m) {
        const uint32_t p = bp::pos(m);
        CHECK(p < 4096u);
        if (p < 4096u) {
            CHECK(inv[p] < 0);
            inv[p] = int(m);
        }
    }
    for (int p = 0; p < 4096; ++p) CHECK(inv[size_t(p)] >= 0);
    // addr[a_hi][c_hi][h][q]: kept for the bank check below
    std::vector<uint32_t> addr(size_t(128) * 128 * 2 * 4);
    for (uint32_t c_hi = 0; c_hi < 128; ++c_hi)
        for (uint32_t h = 0; h < 2; ++h) {
            uint32_t xe = bp::xe0(c_hi, h), xo = bp::xo0(c_hi, h);
            for (uint32_t a_hi = 0; a_hi < 128; ++a_hi) {
                const uint32_t x = a_hi ^ c_hi;
                const uint32_t bs = block_sign_by_definition(a_hi, x, neg_hi);
                CHECK(bs == (bp::sign_uniform(a_hi, neg_hi) ^ bp::parity(c_hi & bp::sign_mask(a_hi, neg_hi))));
                for (uint32_t q = 0; q < 4; ++q) {
                    const uint32_t base = (q & 2u ? xo : xe) + (q & 1u) * bp::kQuadStride;
                    addr[((size_t(a_hi) * 128 + c_hi) * 2 + h) * 4 + q] = base;
                    CHECK(base % 16u == 0 && base + 16u <= 2u * bp::kImageBytes);
                    for (uint32_t e = 0; e < 4; ++e) {
                        const uint32_t byte = base + 4u * e;
                        const uint32_t image = byte / bp::kImageBytes, word = (byte % bp::kImageBytes) / 4u;
                        const uint32_t t = 4u * q + e, k = 2u * bp::s2_of_word(t) + h;
                        CHECK(image < 2u);
                        CHECK(uint32_t(inv[word]) == ((x << 5) | k));
                        CHECK(image == (bs ^ (popc(c_hi) & popc(k) & 1u)));
                    }
                }
                const uint32_t d = bp::delta(step_pattern(a_hi), c_hi, neg_hi) ^ bp::delta_uniform(a_hi, neg_hi);
                xe ^= d;
                xo ^= d;
            }
            CHECK(xe == bp::xe0(c_hi, h) && xo == bp::xo0(c_hi, h));   // where the next item starts
        }
    // banks: wave `tile` holds the columns c_hi = 32 tile + (lane & 31), h = lane >> 5
    for (uint32_t a_hi = 0; a_hi < 128; ++a_hi)
        for (uint32_t tile = 0; tile < 4; ++tile)
            for (uint32_t q = 0; q < 4; ++q) {
                auto at = [&](int lane) {
                    const uint32_t c_hi = (tile << 5) | uint32_t(lane & 31), h = uint32_t(lane >> 5);
                    return addr[((size_t(a_hi) * 128 + c_hi) * 2 + h) * 4 + q];
                };
                for (int g = 0; g < 4; ++g) {
                    uint32_t quads = 0, seen = 0, lo = ~0u;
                    for (int l = 0; l < 16; ++l) quads |= 1u << ((at(kCycleGroups[g][l]) / 16u) % 16u);   // 16 bytes = 4 of the 64 banks
                    CHECK(quads == 0xffffu);
                    for (int l = 0; l < 16; ++l) {   // 16 consecutive lanes, the sign bit set aside
                        const uint32_t a = at(16 * g + l) & ~bp::kNeg;
                        lo = a < lo ? a : lo;
                    }
                    CHECK(lo % 256u == 0);
                    for (int l = 0; l < 16; ++l) {
                        const uint32_t a = at(16 * g + l) & ~bp::kNeg;
                        CHECK(a >= lo && a < lo + 256u);
                        seen |= 1u << ((a - lo) / 16u % 16u);
                    }
                    CHECK(seen == 0xffffu);
                }
            }
    std::printf("%s  header invariants (%s)\n", failures ? "FAILED" : "ok", what);
}

static void plan_images_multiply_right(const double* metric, bool expect_planes, const char* what) {
    const int n = 12;
    const uint64_t full = (uint64_t(2) << n) - 1;
    gaast_expr_t a = gaast_expr_input(0, full, n), b = gaast_expr_input(1, full, n);
    gaast_expr_t e = gaast_expr_product(a, b, GAAST_PROD_GEOMETRIC);
    gaast_spec_t spec = gaast_expr_specialize(e, n, metric, uint64_t(1) << 16);   // (the dense plan needs no comp-mul list)
    CHECK(spec != nullptr);
    if (spec) {
        gaast_program_desc desc;
        CHECK(gaast_spec_program_desc(spec, GAAST_F32, 0, &desc) == 0);
        gaast::Plan plan;
        gaast::build_plan(desc, plan);
        const gaast::Step* st = nullptr;
        for (const gaast::Step& s : plan.steps)
            if (s.kind == gaast::Step::PRODUCT_DENSE) st = &s;
        CHECK(st != nullptr && st->dense.family == gaast::DenseFamily::MFMA32P && st->dense.n == n);
        if (st && st->dense.family == gaast::DenseFamily::MFMA32P) {
            const gaast::Step::Dense& ds = st->dense;
            CHECK((ds.degenerate == 0) == expect_planes);
            const uint32_t N = 1u << n;
            CHECK(ds.left_map.size() == N && ds.right_map.size() == N && !ds.scaled);
            std::vector<int> inv(N, -1);
            for (uint32_t m = 0; m < N; ++m) inv[expect_planes ? bp::pos(m) : gaast::dense_images::mfma32p_b_pos(m)] = int(m);   // (the block image of every other instantiation)
            // images as the staging writes them (+ image; the - image is its negation), exact small integers
            std::vector<double> lrow(N), rrow(N), Aimg(N, 0.0), Bimg(N, 0.0), Bblade(N, 0.0);
            uint64_t x = 88172645463325252ULL;
            auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return double(int(x % 17) - 8); };
            for (double& v : lrow) v = rnd();
            for (double& v : rrow) v = rnd();
            std::vector<char> hit(N, 0);
            for (uint32_t w : ds.left_map) Aimg[(w >> 16) & 0x7fffu] = (w >> 31) ? -lrow[w & 0xffffu] : lrow[w & 0xffffu];
            for (uint32_t w : ds.right_map) {
                const uint32_t p = (w >> 16) & 0x7fffu;
                CHECK(p < N && !hit[p < N ? p : 0]);
                if (p >= N) continue;
                hit[p] = 1;
                Bimg[p] = (w >> 31) ? -rrow[w & 0xffffu] : rrow[w & 0xffffu];
                const uint32_t blade = uint32_t(inv[p]);   // the host folds (-1)^(|b_hi| |b_lo|) into the image: taken out for the formula
                Bblade[blade] = (popc(blade >> 5) & popc(blade & 31u) & 1u) ? -Bimg[p] : Bimg[p];
            }
            if (expect_planes) {
                const uint32_t cols[6] = {0, 1, 37, 64 + 26, 96 + 21, 127};
                size_t bad = 0;
                for (uint32_t c_hi : cols) {
                    // the two lanes (c_hi, h) walk their B addresses; Bk[a_hi][k]: the word the lane of parity k & 1 multiplies
                    std::vector<double> Bk(size_t(128) * 32);
                    for (uint32_t h = 0; h < 2; ++h) {
                        uint32_t xe = bp::xe0(c_hi, h), xo = bp::xo0(c_hi, h);
                        for (uint32_t a_hi = 0; a_hi < 128; ++a_hi) {
                            for (uint32_t t = 0; t < 16; ++t) {
                                const uint32_t byte = ((t >> 2) & 2u ? xo : xe) + ((t >> 2) & 1u) * bp::kQuadStride + 4u * (t & 3u);
                                const double v = Bimg[(byte % bp::kImageBytes) / 4u];
                                Bk[a_hi * 32 + 2 * bp::s2_of_word(t) + h] = byte / bp::kImageBytes ? -v : v;
                            }
                            const uint32_t d = bp::delta(step_pattern(a_hi), c_hi, ds.neg_hi) ^ bp::delta_uniform(a_hi, ds.neg_hi);
                            xe ^= d;
                            xo ^= d;
                        }
                    }
                    for (uint32_t r = 0; r < 32; ++r) {
                        double got = 0.0, want = 0.0;
                        for (uint32_t a_hi = 0; a_hi < 128; ++a_hi)
                            for (uint32_t k = 0; k < 32; ++k) {
                                const uint32_t a_lo = r ^ k;
                                uint32_t par = popc(a_lo & k & ds.neg_lo) & 1u;   // the kernel's lane-constant A sign
                                for (int pp = 1; pp < 5; ++pp)
                                    if ((a_lo >> pp) & 1u) par ^= popc(k & ((1u << pp) - 1u)) & 1u;
                                const double av = Aimg[(a_hi << 5) | a_lo];
                                got += (par ? -av : av) * Bk[a_hi * 32 + k];
                                // the plain formula in the permuted basis
                                const uint32_t pa = (a_hi << 5) | a_lo, pb = ((a_hi ^ c_hi) << 5) | k;
                                uint32_t s = 0;
                                for (int p = 1; p < n; ++p)
                                    if ((pa >> p) & 1u) s ^= popc(pb & ((1u << p) - 1u)) & 1u;
                                s ^= popc(pa & pb & 31u & ds.neg_lo) & 1u;
                                s ^= popc(((pa & pb) >> 5) & ds.neg_hi) & 1u;
                                want += (s ? -1.0 : 1.0) * Aimg[pa] * Bblade[pb];
                            }
                        bad += got != want;
                    }
                }
                if (bad) std::printf("%s: %zu result components differ\n", what, bad);
                CHECK(bad == 0);
            }
        }
        gaast_spec_free(spec);
    }
    gaast_expr_release(e);
    gaast_expr_release(b);
    gaast_expr_release(a);
    std::printf("%s  %s\n", failures ? "FAILED" : "ok", what);
}

int main() {
    header_invariants(0u, "Euclidean");
    header_invariants(0x4bu, "hi vectors 0, 1, 3, 6 square to -1");
    const double euclid[12] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    const double mixed[12] = {1, -1, 1, 1, -1, 1, -1, 1, 1, -1, -1, 1};   // -1 among the lo and among the hi vectors
    const double null_hi[12] = {1, 1, -1, 1, 1, 1, 1, 0, 1, -1, 1, 1};    // a null vector: the degenerate instantiation keeps the block image
    plan_images_multiply_right(euclid, true, "plan + images, R^12");
    plan_images_multiply_right(mixed, true, "plan + images, mixed signature");
    plan_images_multiply_right(null_hi, false, "plan, one null vector: block image");
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
