// The list chain specialised per program: its tables and layout (chain_tables), and its hiprtc source (chain_source).  The generated
// text and tables are pinned byte for byte by tests/test_codegen_digests.py.
#include "plan_internal.hpp"

#include <algorithm>

namespace gaast {
namespace {

// what chain_tables decides and chain_source spells out as the kernel's compile-time constants (lengths and offsets in elements)
struct ChainShape {
    int64_t esz, threads, ipb, stride, l1, r1, r2, mid, neg_len, off_l1, off_r1, off_neg, off_mid, off_r2, off_zero, rows1, w1, w1s, rows2, w2, w2p, wps, wms, wss, split, ent2_at, ent1_at, used;
    int alias, side, ent2_mode, ent1_mode;
    bool neg_is_left, covered, single, has_init, xreg, sorted;
};

// tolerance mode: list 2 sign-sorted (below) -- when the item still fits the 16-bit byte offsets with one more element, and the
// rows' signs are balanced enough: every (row, slice) pair is padded to the longest plus and the longest minus segment, and a
// padding term costs what a real one does (Euclidean sandwiches at n = 8, 10 have all-plus rows: +50 % terms -- they keep the
// sign words; R^{6,3} at n = 9: 64 + 64 of 128, no padding; (a + b c).g(2) at n = 8: 136 + 136 for 256)
bool sign_sorted_pays(const Plan& plan, const Step& c, int64_t mid) {
    const int64_t rows2e = int64_t(c.list.row_out.size()), w2e = c.list.ell_width;
    // ("make_chain_jit in XREG mode ...", second point: this pre-check assumes ipb = 32, the final split uses the final ipb)
    int64_t sp = 1;   // (the slice count of the tolerance mode, decided again below with the same rule)
    while (sp < 4 && w2e % (2 * sp) == 0 && w2e / (2 * sp) >= 32 && rows2e * 32 * 2 * sp <= 1024 && rows2e * 2 * sp <= mid) sp *= 2;
    const int64_t gran = plan.dtype == GAAST_F32 ? 16 : 8;
    int64_t wp = 0, wm = 0;
    for (int64_t row = 0; row < rows2e; ++row) {
        int64_t np = 0, nm = 0;
        for (int64_t t = 0; t < w2e; ++t) ((c.list.entries[size_t(t * rows2e + row)] & 0x80000000u) ? nm : np) += 1;
        wp = std::max(wp, (np + sp - 1) / sp);
        wm = std::max(wm, (nm + sp - 1) / sp);
    }
    wp = (wp + gran - 1) / gran * gran;
    wm = (wm + gran - 1) / gran * gran;
    return rows2e > 0 && w2e > 0 && (wp + wm) * sp * 100 <= w2e * 107;
}

// The layout of an item in LDS, where the tables ride, the workgroup size, and the tables themselves (c.cj.ent1 / pos1 / ent2 / out2).
// false: the chain does not fit the kernel's formats (c.cj stays off).
bool chain_tables(const Plan& plan, Step& c, const Step& w, bool single, int64_t l1, int64_t r1, int64_t mid, int64_t r2, int alias, int side, bool covered,
                  const std::vector<uint32_t>* init_off, ChainShape& sh) {
    const int64_t esz = plan.dtype == GAAST_F32 ? 4 : 8;
    const int64_t neg_len = single ? 0 : std::min(l1, r1);
    const bool neg_is_left = l1 < r1;
    // layout of an item in LDS (elements): list 2's own operand first (its offsets have 15 bits), then the rest
    int64_t off_l1 = 0, off_r1 = 0, off_neg, off_mid, off_r2 = -1, cur = 0;
    auto place = [&](int64_t len) { const int64_t o = cur; cur += len; return o; };
    if (alias == 0) off_r2 = place(r2);
    if (alias == 2) { off_r1 = place(r1); off_l1 = place(l1); }
    else { off_l1 = place(l1); off_r1 = place(r1); }
    off_neg = place(neg_len);
    off_mid = place(mid);
    const bool sorted = !(plan.flags & GAAST_FLAG_EXACT_ORDER) && (cur + 1) * esz <= 65536 && sign_sorted_pays(plan, c, mid);
    const bool has_zero = !(plan.flags & GAAST_FLAG_EXACT_ORDER) && (cur + 1) * esz <= 65536;
    const int64_t off_zero = has_zero ? place(1) : 0;             // ... padding terms (sorted list 2, list 1 by right index) multiply this element
    int64_t stride = cur | 1;   // odd: lanes reading one offset of consecutive items touch consecutive banks (bank pairs in f64)
    const int64_t off_other = alias == 0 ? off_r2 : alias == 1 ? off_l1 : off_r1;
    const int64_t other_len = alias == 0 ? r2 : alias == 1 ? l1 : r1;
    if ((off_other + other_len) * esz > 32768 || cur * esz > 65536) return false;   // (15-bit / 16-bit byte offsets from the item's base)
    const int64_t rows1 = int64_t(w.list.row_out.size()), rows2 = int64_t(c.list.row_out.size());
    const int64_t w1 = w.list.ell_width, w2 = c.list.ell_width;
    if (rows2 <= 0 || w2 <= 0) return false;
    if (!single && (rows1 <= 0 || w1 <= 0 || w1 > 32)) return false;   // (list 1's operands of a row are all in flight at once)
    // items per workgroup: a power of two up to 32 (the lanes of an LDS access group), as many as the LDS holds
    int64_t ipb = 32;
    const int64_t lds_cap = int64_t(kLdsBytes);
    while (ipb > 1 && ipb * stride * esz > lds_cap - 4096) ipb >>= 1;
    if (ipb < 2) return false;
    const int64_t w1p = (w1 + 3) & ~int64_t(3), w2p = (w2 + 3) & ~int64_t(3);
    // The tables ride in LDS when they fit beside the items (broadcast reads; from global memory every lane would get its own
    // copy of the words through the vector cache: 16 cycles of its return path per 16-byte load and wave).
    //   list 2: WIDE entries (8 bytes: [15:0] mid | [31:16] other, then the sign bit alone) cost two vector instructions less per
    //           term than narrow ones ([15:0] mid | [30:16] other | [31] sign) -- taken when they fit;
    //   list 1: rows padded to quads (16-byte reads) when that fits, else unpadded rows (4-byte reads), else global memory.
    const int64_t items_bytes = (ipb * stride * esz + 15) / 16 * 16;
    int64_t used = items_bytes;
    // TOLERANCE MODE, SIGN-SORTED (round 4): the order inside a row is free, so the terms of every (row, slice) pair are stored
    // plus-terms first (padded to WPS), then minus-terms (padded to WMS): the sign is the POSITION -- no sign word, no sign
    // instruction: a term is two SDWA address additions and one fused multiply-add (exact order: 5, narrow entries: 7) -- and the
    // entries are clean 16 + 16-bit words (half the wide table: at n = 9 list 1's table then fits in LDS too).  Padding terms
    // multiply the item's zero element by itself.  The slice count is decided first (it shapes the table).
    int64_t split = 1;
    if (!(plan.flags & GAAST_FLAG_EXACT_ORDER))
        while (split < 4 && w2 % (2 * split) == 0 && w2 / (2 * split) >= 32 && rows2 * ipb * 2 * split <= 1024 && rows2 * 2 * split <= mid) split *= 2;
    int64_t wps = 0, wms = 0;   // plus / minus terms per (row, slice), multiples of 8 (f32: 16): whole register batches
    std::vector<std::vector<uint32_t>> plus_terms, minus_terms;   // per row: mid offset | other offset << 16 (bytes)
    if (sorted) {
        plus_terms.resize(size_t(rows2));
        minus_terms.resize(size_t(rows2));
        const int64_t off_other_b = (alias == 0 ? off_r2 : alias == 1 ? off_l1 : off_r1) * esz;
        for (int64_t row = 0; row < rows2; ++row)
            for (int64_t t = 0; t < w2; ++t) {
                const uint32_t e = c.list.entries[size_t(t * rows2 + row)];
                const int64_t lo = e & 0x7fffu, ro = (e >> 16) & 0x7fffu;
                const int64_t ma = off_mid * esz + (side == 1 ? lo : ro), oa = off_other_b + (side == 1 ? ro : lo);
                ((e & 0x80000000u) ? minus_terms : plus_terms)[size_t(row)].push_back(uint32_t(ma) | (uint32_t(oa) << 16));
            }
        const int64_t gran = plan.dtype == GAAST_F32 ? 16 : 8;
        for (int64_t row = 0; row < rows2; ++row) {
            wps = std::max<int64_t>(wps, (int64_t(plus_terms[size_t(row)].size()) + split - 1) / split);
            wms = std::max<int64_t>(wms, (int64_t(minus_terms[size_t(row)].size()) + split - 1) / split);
        }
        wps = (wps + gran - 1) / gran * gran;
        wms = (wms + gran - 1) / gran * gran;
    }
    const int64_t wss = wps + wms;
    int ent2_mode;   // 0: narrow, global; 1: narrow, LDS; 2: wide, LDS; sorted: 3: LDS, 4: global
    if (sorted) {
        if (used + rows2 * split * wss * 4 <= lds_cap) ent2_mode = 3, used += rows2 * split * wss * 4;
        else ent2_mode = 4;
    } else if (used + rows2 * w2p * 8 <= lds_cap) ent2_mode = 2, used += rows2 * w2p * 8;
    else if (used + rows2 * w2p * 4 <= lds_cap) ent2_mode = 1, used += rows2 * w2p * 4;
    else ent2_mode = 0;
    const int64_t ent2_at = items_bytes;
    int ent1_mode;   // 0: padded rows, global; 1: unpadded rows, LDS; 2: padded rows, LDS
    const int64_t ent1_at = used;
    if (used + rows1 * w1p * 4 <= lds_cap) ent1_mode = 2, used += rows1 * w1p * 4;
    else if (used + rows1 * w1 * 4 <= lds_cap) ent1_mode = 1, used += rows1 * w1 * 4;
    else ent1_mode = 0;
    used = (used + 15) / 16 * 16;
    // TOLERANCE MODE (without GAAST_FLAG_EXACT_ORDER, like the dense products): a long row of list 2 is cut into `split` slices of
    // consecutive terms, each summed by a lane of its own in the reference's order, the partial sums added in slice order at the end --
    // the few long chains that leave most of the workgroup idle become split x as many, half as long.  |error| <= 4 eps sum |terms|
    // per component (the dense path's contract; one extra rounding per slice).  GAAST_FLAG_EXACT_ORDER: split = 1, bit for bit.
    // one workgroup per CU (the usual case from n = 9 on): 512 threads -- list 1 and the staging have work for all of them, list 2
    // (few long rows) for rows2 * split * ipb lanes; two or more workgroups per CU: 256 threads each
    int64_t threads = 2 * used <= lds_cap ? 256 : 512;
    threads = std::max<int64_t>(threads, std::min<int64_t>(1024, (rows2 * split * ipb + 63) / 64 * 64));
    // whole multiples of 256: the waves of a workgroup are dealt round-robin to the CU's four SIMDs, and every phase ends at a
    // barrier -- 9 or 10 waves leave one SIMD with three where the others have two (measured: sand9g1 576 -> 768 threads +6 %,
    // sand10g1 640 -> 768 +2 %; 1,024 where list 2 does not ask for them: -3 % / -23 %)
    threads = std::min<int64_t>(1024, (threads + 255) / 256 * 256);
    const int64_t w1s = ent1_mode == 1 ? w1 : w1p;   // words per row of list 1's table
    // tables
    // TOLERANCE MODE, list 1 with its small right operand IN REGISTERS (the sandwich's X: n components, the same for every row a lane
    // evaluates): the terms of a row are re-ordered by right index -- term j multiplies by x_j, a register --, so a term is ONE LDS
    // read (the left operand), its sign a bit of the table word; rows without a term for some j multiply the item's zero element.
    // ("make_chain_jit in XREG mode ...", first point: the padding term 0 * x_j is not masked)
    bool xreg = has_zero && !single && !neg_is_left && r1 <= 12 && w1 <= r1 && ent1_mode != 1 && w1s >= ((r1 + 3) & ~int64_t(3));
    for (int64_t row = 0; row < rows1 && xreg; ++row) {
        uint32_t seen = 0;
        for (int64_t t = 0; t < w1 && xreg; ++t) {
            const int64_t j = int64_t((w.list.entries[size_t(t * rows1 + row)] >> 16) & 0x7fffu) / esz;
            xreg = j < r1 && !(seen & (1u << j));
            seen |= 1u << j;
        }
    }
    c.cj.ent1.assign(size_t(rows1 * w1s), 0u);
    c.cj.pos1.resize(size_t(rows1));
    if (init_off) c.cj.pos1 = *init_off;   // (a single list has no row positions: the slot carries the offsets of the folded copy)
    for (int64_t row = 0; row < rows1; ++row) {
        c.cj.pos1[size_t(row)] = uint32_t((off_mid + int64_t(w.list.row_out[size_t(row)])) * esz);
        for (int64_t t = 0; t < w1; ++t) {
            const uint32_t e = w.list.entries[size_t(t * rows1 + row)];
            const bool neg = (e & 0x80000000u) != 0;
            const int64_t lo = e & 0x7fffu, ro = (e >> 16) & 0x7fffu;   // bytes, from the operand rows
            const int64_t la = ((neg && neg_is_left) ? off_neg : off_l1) * esz + lo;
            const int64_t ra = ((neg && !neg_is_left) ? off_neg : off_r1) * esz + ro;
            if (!xreg) c.cj.ent1[size_t(row * w1s + t)] = uint32_t(la) | (uint32_t(ra) << 16);
        }
        if (xreg) {
            for (int64_t j = 0; j < w1s; ++j) c.cj.ent1[size_t(row * w1s + j)] = uint32_t(off_zero * esz);   // no term for x_j: 0 * x_j
            for (int64_t t = 0; t < w1; ++t) {
                const uint32_t e = w.list.entries[size_t(t * rows1 + row)];
                const int64_t lo = e & 0x7fffu, j = int64_t((e >> 16) & 0x7fffu) / esz;
                c.cj.ent1[size_t(row * w1s + j)] = uint32_t(off_l1 * esz + lo) | (e & 0x80000000u);
            }
        }
    }
    const int64_t wpt2 = ent2_mode == 2 ? 2 : 1;   // words per term
    c.cj.out2 = c.list.row_out;
    if (sorted) {
        const uint32_t pad = uint32_t(off_zero * esz) | (uint32_t(off_zero * esz) << 16);
        c.cj.ent2.assign(size_t(rows2 * split * wss), pad);
        for (int64_t row = 0; row < rows2; ++row)
            for (int which = 0; which < 2; ++which) {
                const std::vector<uint32_t>& tv = which ? minus_terms[size_t(row)] : plus_terms[size_t(row)];
                const int64_t per = (int64_t(tv.size()) + split - 1) / split;   // consecutive chunks, one per slice
                for (int64_t i = 0; i < int64_t(tv.size()); ++i) {
                    const int64_t sl = per ? i / per : 0, k = per ? i % per : 0;
                    c.cj.ent2[size_t((row * split + sl) * wss + (which ? wps : 0) + k)] = tv[size_t(i)];
                }
            }
    } else
        c.cj.ent2.assign(size_t(rows2 * w2p * wpt2), 0u);
    for (int64_t row = 0; row < rows2 && !sorted; ++row)
        for (int64_t t = 0; t < w2; ++t) {
            const uint32_t e = c.list.entries[size_t(t * rows2 + row)];
            const int64_t lo = e & 0x7fffu, ro = (e >> 16) & 0x7fffu;
            const int64_t ma = off_mid * esz + (side == 1 ? lo : ro), oa = off_other * esz + (side == 1 ? ro : lo);
            if (ent2_mode == 2) {
                c.cj.ent2[size_t((row * w2p + t) * 2)] = uint32_t(ma) | (uint32_t(oa) << 16);
                c.cj.ent2[size_t((row * w2p + t) * 2 + 1)] = e & 0x80000000u;
            } else {
                c.cj.ent2[size_t(row * w2p + t)] = uint32_t(ma) | (uint32_t(oa) << 16) | (e & 0x80000000u);
            }
        }
    sh.esz = esz; sh.threads = threads; sh.ipb = ipb; sh.stride = stride; sh.l1 = l1; sh.r1 = r1;
    sh.r2 = r2; sh.mid = mid; sh.neg_len = neg_len; sh.off_l1 = off_l1; sh.off_r1 = off_r1; sh.off_neg = off_neg;
    sh.off_mid = off_mid; sh.off_r2 = off_r2; sh.off_zero = off_zero; sh.rows1 = rows1; sh.w1 = w1; sh.w1s = w1s;
    sh.rows2 = rows2; sh.w2 = w2; sh.w2p = w2p; sh.wps = wps; sh.wms = wms; sh.wss = wss;
    sh.split = split; sh.ent2_at = ent2_at; sh.ent1_at = ent1_at; sh.used = used; sh.alias = alias; sh.side = side;
    sh.ent2_mode = ent2_mode; sh.ent1_mode = ent1_mode; sh.neg_is_left = neg_is_left; sh.covered = covered; sh.single = single; sh.xreg = xreg;
    sh.sorted = sorted; sh.has_init = init_off != nullptr;
    return true;
}

// the kernel: every size, offset and mode above is a #define ahead of this text
const char kChainKernel[] = R"JIT(
typedef unsigned int u32;
typedef unsigned long long u64;
typedef u32 u32x4 __attribute__((ext_vector_type(4)));
typedef T VT __attribute__((ext_vector_type(16 / ESZ)));
#define EPC (16 / ESZ)
#if F64
#define ONE_HI 0x3ff00000u
__device__ __forceinline__ T with_hi(T v, u32 hi) { return __builtin_bit_cast(double, (u64(hi) << 32) | (__builtin_bit_cast(u64, v) & 0xffffffffull)); }
__device__ __forceinline__ u32 hi_of(T v) { return u32(__builtin_bit_cast(u64, v) >> 32); }
__device__ __forceinline__ T pm_one(u32 hi) { return __builtin_bit_cast(double, u64(hi) << 32); }
#define FMA(a, b, c) __builtin_fma(a, b, c)
#else
#define ONE_HI 0x3f800000u
__device__ __forceinline__ T with_hi(T v, u32 hi) { return __builtin_bit_cast(float, hi); }
__device__ __forceinline__ u32 hi_of(T v) { return __builtin_bit_cast(u32, v); }
__device__ __forceinline__ T pm_one(u32 hi) { return __builtin_bit_cast(float, hi); }
#define FMA(a, b, c) __builtin_fmaf(a, b, c)
#endif
#if EXACT
#define MAC(a, b, c) ((c) + (a) * (b))
#else
#define MAC(a, b, c) FMA(a, b, c)
#endif
typedef __attribute__((address_space(3))) unsigned char lds_u8;
#define LDS(addr) (*(const __attribute__((address_space(3))) T*)(smem + (addr)))

// operand rows of the group's items, element e = item * LEN + c of the flattened range; rows beyond the batch are zero
template <int LEN, int CANON, int OFF, int NEGOFF>
__device__ __forceinline__ void put(lds_u8* smem, int e, T v) {
    const int i2 = e / LEN, c = e - i2 * LEN;
    if (CANON) v = T(0) + v;                                      // init_null_mv + add_grades_from: 0.0 + x (eval.rs:27-31)
    *(__attribute__((address_space(3))) T*)(smem + i2 * STRIDE_B + OFF + c * ESZ) = v;
    if (NEGOFF >= 0) *(__attribute__((address_space(3))) T*)(smem + i2 * STRIDE_B + NEGOFF + c * ESZ) = -v;
}
template <int LEN, int CANON, int OFF, int NEGOFF>
__device__ __forceinline__ void stage(lds_u8* smem, const T* __restrict__ src, long long stride, long long item0, int nitems, int tid) {
    constexpr int TOTAL = IPB * LEN;
#pragma unroll 4
    for (int e = tid; e < TOTAL; e += NT) {
        const int i2 = e / LEN, c = e - i2 * LEN;
        put<LEN, CANON, OFF, NEGOFF>(smem, e, i2 < nitems ? src[(item0 + i2) * stride + c] : T(0));
    }
}
// ... the same rows as 16-byte pieces through registers: issued for the NEXT group while the current one is evaluated (contiguous,
// 16-byte aligned rows of a full group; anything else takes stage())
template <int LEN>
struct Pre {
    static constexpr int NCH = IPB * LEN / EPC, CPT = (NCH + NT - 1) / NT;
    VT v[CPT];
    __device__ __forceinline__ void issue(const T* __restrict__ src, long long item0, int tid) {
        const VT* s16 = (const VT*)(src + item0 * LEN);
#pragma unroll
        for (int k = 0; k < CPT; ++k)
            if (tid + k * NT < NCH) v[k] = __builtin_nontemporal_load(s16 + tid + k * NT);
    }
    template <int CANON, int OFF, int NEGOFF>
    __device__ __forceinline__ void commit(lds_u8* smem, int tid) {
#pragma unroll
        for (int k = 0; k < CPT; ++k)
            if (tid + k * NT < NCH) {
#pragma unroll
                for (int j = 0; j < EPC; ++j) put<LEN, CANON, OFF, NEGOFF>(smem, (tid + k * NT) * EPC + j, v[k][j]);
            }
    }
};

extern "C" __global__ __launch_bounds__(NT) void gaast_chain(const T* __restrict__ l1, long long s_l1, const T* __restrict__ r1, long long s_r1,
                                                              const T* __restrict__ r2, long long s_r2, T* __restrict__ out, long long s_out,
                                                              const u32* __restrict__ ent1, const u32* __restrict__ pos1,
                                                              const u32* __restrict__ ent2, const u32* __restrict__ out2, long long batch,
                                                              const T* __restrict__ init, long long s_init) {
    __shared__ __attribute__((aligned(16))) unsigned char smem_raw[SMEM_BYTES];
    lds_u8* smem = (lds_u8*)smem_raw;
    const int tid = threadIdx.x;
    const int it = tid & (IPB - 1), sub = tid / IPB;
    const u32 base = u32(it) * STRIDE_B;
    u32 one_hi = ONE_HI;
    asm volatile("" : "+v"(one_hi));   // a vector register (the and-or takes one scalar operand)
    // the tables, once per (persistent) workgroup
#if SORTED || XREG
    for (int e = tid; e < IPB; e += NT) *(__attribute__((address_space(3))) T*)(smem + e * STRIDE_B + OFF_ZERO) = T(0);   // the padding terms' operand
#endif
#if ENT2_MODE == 3
    for (int e = tid; e < ROWS2 * SPLIT * WSS / 4; e += NT) ((__attribute__((address_space(3))) u32x4*)(smem + ENT2_AT))[e] = ((const u32x4*)ent2)[e];
#elif ENT2_MODE == 2
    for (int e = tid; e < ROWS2 * W2P / 2; e += NT) ((__attribute__((address_space(3))) u32x4*)(smem + ENT2_AT))[e] = ((const u32x4*)ent2)[e];
#elif ENT2_MODE == 1
    for (int e = tid; e < ROWS2 * W2P / 4; e += NT) ((__attribute__((address_space(3))) u32x4*)(smem + ENT2_AT))[e] = ((const u32x4*)ent2)[e];
#endif
#if ENT1_MODE >= 1 && !SINGLE
    for (int e = tid; e < ROWS1 * W1S; e += NT) ((__attribute__((address_space(3))) u32*)(smem + ENT1_AT))[e] = ent1[e];
#endif
    // entry words: list 1, term t of `row`; list 2, the quad holding terms 4q .. 4q + 3 (narrow) / 2q, 2q + 1 (wide)
#if !SINGLE
    auto ent1_quad = [&](int row, int q) -> u32x4 {
#if ENT1_MODE == 2
        return ((const __attribute__((address_space(3))) u32x4*)(smem + ENT1_AT))[row * (W1S / 4) + q];
#elif ENT1_MODE == 1
        const __attribute__((address_space(3))) u32* pw = (const __attribute__((address_space(3))) u32*)(smem + ENT1_AT) + row * W1S + 4 * q;
        u32x4 r;
        r[0] = pw[0];
        r[1] = 4 * q + 1 < W1 ? pw[1] : 0u;
        r[2] = 4 * q + 2 < W1 ? pw[2] : 0u;
        r[3] = 4 * q + 3 < W1 ? pw[3] : 0u;
        return r;
#else
        return ((const u32x4*)ent1)[row * (W1S / 4) + q];
#endif
    };
#endif
    auto ent2_quad = [&](int row, int q) -> u32x4 {
#if ENT2_MODE == 2
        return ((const __attribute__((address_space(3))) u32x4*)(smem + ENT2_AT))[row * (W2P / 2) + q];
#elif ENT2_MODE == 1
        return ((const __attribute__((address_space(3))) u32x4*)(smem + ENT2_AT))[row * (W2P / 4) + q];
#else
        return ((const u32x4*)ent2)[row * (W2P / 4) + q];
#endif
    };
    u32 oo_reg[PASSES2];   // this thread's rows of list 2: their output offsets, loaded once
#pragma unroll
    for (int k = 0; k < PASSES2; ++k) oo_reg[k] = sub + k * NSUB < ROWS2 * SPLIT ? out2[(sub + k * NSUB) / SPLIT] : 0u;
#if INIT_SRC
    u32 io_reg[PASSES2];   // ... and where their accumulators start from: 0.0 + init[offset] (a covering copy_grades_from folded in)
#pragma unroll
    for (int k = 0; k < PASSES2; ++k) io_reg[k] = sub + k * NSUB < ROWS2 * SPLIT ? pos1[(sub + k * NSUB) / SPLIT] : 0u;
#endif
    const long long groups = (batch + IPB - 1) / IPB;
    // register-prefetch staging needs contiguous, 16-byte aligned rows (wave-uniform test); shared rows (stride 0), wrapped
    // strided memory and the last, partial group take the plain loop
    // (the memory counter is IN ORDER: a wait for any later global load would wait for the prefetched rows first, so the evaluation
    //  issues none where it can: row positions and output offsets in registers, tables in LDS.  A table that has to stay in global
    //  memory (n = 10: list 1's) makes the first row of list 1 wait for the prefetch -- still better than no prefetch: measured
    //  0.214 against 0.164 G items/s at n = 10)
#if SINGLE
    // a single list: the left operand is the staged "mid" row (pointer l1), the right one list 2's own operand (pointer r2)
    const bool fast = s_l1 == MID && s_r2 == R2 && ((u64)l1 & 15ull) == 0 && ((u64)r2 & 15ull) == 0 && (IPB * MID) % EPC == 0 && (IPB * R2) % EPC == 0;
    Pre<MID> pl;
    Pre<R2> pq;
    auto issue = [&](long long item0) {
        pl.issue(l1, item0, tid);
        pq.issue(r2, item0, tid);
    };
    auto commit = [&]() {
        pl.template commit<CANON_MID, OFF_MID, -1>(smem, tid);
        pq.template commit<CANON_R2, OFF_R2, -1>(smem, tid);
    };
    auto stage_all = [&](long long item0, int nitems) {
        stage<MID, CANON_MID, OFF_MID, -1>(smem, l1, s_l1, item0, nitems, tid);
        stage<R2, CANON_R2, OFF_R2, -1>(smem, r2, s_r2, item0, nitems, tid);
    };
#else
    const bool fast = s_l1 == L1 && s_r1 == R1 && ((u64)l1 & 15ull) == 0 && ((u64)r1 & 15ull) == 0 && (IPB * L1) % EPC == 0 && (IPB * R1) % EPC == 0
#if HAS_R2
                      && s_r2 == R2 && ((u64)r2 & 15ull) == 0 && (IPB * R2) % EPC == 0
#endif
        ;
    Pre<L1> pl;
    Pre<R1> pr;
#if HAS_R2
    Pre<R2> pq;
#endif
    auto issue = [&](long long item0) {
        pl.issue(l1, item0, tid);
        pr.issue(r1, item0, tid);
#if HAS_R2
        pq.issue(r2, item0, tid);
#endif
    };
    auto commit = [&]() {
        pl.template commit<CANON_L1, OFF_L1, (NEG_IS_LEFT ? OFF_NEG : -1)>(smem, tid);
        pr.template commit<CANON_R1, OFF_R1, (NEG_IS_LEFT ? -1 : OFF_NEG)>(smem, tid);
#if HAS_R2
        pq.template commit<CANON_R2, OFF_R2, -1>(smem, tid);
#endif
    };
    auto stage_all = [&](long long item0, int nitems) {
        stage<L1, CANON_L1, OFF_L1, (NEG_IS_LEFT ? OFF_NEG : -1)>(smem, l1, s_l1, item0, nitems, tid);
        stage<R1, CANON_R1, OFF_R1, (NEG_IS_LEFT ? -1 : OFF_NEG)>(smem, r1, s_r1, item0, nitems, tid);
#if HAS_R2
        stage<R2, CANON_R2, OFF_R2, -1>(smem, r2, s_r2, item0, nitems, tid);
#endif
    };
#endif
    long long g = blockIdx.x;
    if (g >= groups) return;
    {
        const long long item0 = g * IPB;
        const int nitems = int(batch - item0 < IPB ? batch - item0 : IPB);
        if (fast && nitems == IPB) {
            issue(item0);
            commit();
        } else {
            stage_all(item0, nitems);
        }
    }
    for (;;) {   // persistent workgroups
        const long long item0 = g * IPB;
        const int nitems = int(batch - item0 < IPB ? batch - item0 : IPB);
        const long long gn = g + gridDim.x;
        const bool more = gn < groups;
        const int nnext = more ? int(batch - gn * IPB < IPB ? batch - gn * IPB : IPB) : 0;
        const bool pre_next = fast && more && nnext == IPB;
#if !COVERED && !SINGLE
        for (int e = tid; e < IPB * MID; e += NT) *(__attribute__((address_space(3))) T*)(smem + (e / MID) * STRIDE_B + OFF_MID + (e % MID) * ESZ) = T(0);
#endif
        __syncthreads();
#if BETA
        T acc0[PASSES2];   // list 2 adds into what another arm left in `out`: read BEFORE the prefetch is issued (in-order counter)
#pragma unroll
        for (int k = 0; k < PASSES2; ++k) acc0[k] = (sub + k * NSUB < ROWS2 * SPLIT && it < nitems) ? out[(item0 + it) * s_out + oo_reg[k]] : T(0);
#elif INIT_SRC
        T acc0[PASSES2];   // ... or onto a copy of an input's grades, made here: 0.0 + x (graded.rs:195-201 then :74)
#pragma unroll
        for (int k = 0; k < PASSES2; ++k) acc0[k] = T(0) + ((sub + k * NSUB < ROWS2 * SPLIT && it < nitems) ? init[(item0 + it) * s_init + io_reg[k]] : T(0));
#endif
        if (pre_next) issue(gn * IPB);   // in flight while this group is evaluated
        // ---- list 1 -> mid (eval.rs:77-83 into the fresh cache buffer of eval.rs:21-33): the operands of row k + 1 are in
        // flight while row k's chain is evaluated (two register sets, the loop unrolled by two: no copies) ----
#if !SINGLE
#if XREG
        {   // list 1 with the right operand (R1 components of THIS lane's item) in registers: term j of every row multiplies by xr[j]
            T xr[R1];
#pragma unroll
            for (int j = 0; j < R1; ++j) xr[j] = LDS(base + OFF_R1 + j * ESZ);
            T la[R1], lb[R1];
            u32 ea[R1], eb[R1];
            auto load1 = [&](T (&lv)[R1], u32 (&ev)[R1], int row) {
#pragma unroll
                for (int q = 0; q < (R1 + 3) / 4; ++q) {
                    const u32x4 e4 = ent1_quad(row, q);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (4 * q + j < R1) {
                            lv[4 * q + j] = LDS(base + (e4[j] & 0xffffu));
                            ev[4 * q + j] = e4[j];
                        }
                }
            };
            auto sum1 = [&](const T (&lv)[R1], const u32 (&ev)[R1], int row) {
                T acc = T(0);
#pragma unroll
                for (int t = 0; t < R1; ++t) acc = FMA(with_hi(lv[t], hi_of(lv[t]) ^ (ev[t] & 0x80000000u)), xr[t], acc);
#if POS1_LINEAR
                *(__attribute__((address_space(3))) T*)(smem + base + OFF_MID + row * ESZ) = CANON_MID ? T(0) + acc : acc;
#else
                *(__attribute__((address_space(3))) T*)(smem + base + pos1[row]) = CANON_MID ? T(0) + acc : acc;
#endif
            };
            constexpr int LAST1 = ROWS1 - 1;
            int row = sub;
            if (row < ROWS1) load1(la, ea, row);
#pragma nounroll
            for (; row < ROWS1; row += 2 * NSUB) {
                const int r2_ = row + NSUB, r3_ = row + 2 * NSUB;
                load1(lb, eb, r2_ < ROWS1 ? r2_ : LAST1);
                sum1(la, ea, row);
                load1(la, ea, r3_ < ROWS1 ? r3_ : LAST1);
                if (r2_ < ROWS1) sum1(lb, eb, r2_);
            }
        }
        __syncthreads();
#elif !SINGLE
        {
            T la[W1], ra[W1], lb[W1], rb[W1];
            auto load1 = [&](T (&lv)[W1], T (&rv)[W1], int row) {
#pragma unroll
                for (int q = 0; q < (W1 + 3) / 4; ++q) {
                    const u32x4 e4 = ent1_quad(row, q);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (4 * q + j < W1) {
                            lv[4 * q + j] = LDS(base + (e4[j] & 0xffffu));
                            rv[4 * q + j] = LDS(base + (e4[j] >> 16));
                        }
                }
            };
            auto sum1 = [&](const T (&lv)[W1], const T (&rv)[W1], int row) {
                T acc = T(0);
#pragma unroll
                for (int t = 0; t < W1; ++t) acc = MAC(lv[t], rv[t], acc);   // (l * r) * (+-1) then +=: the sign rides in the image
#if POS1_LINEAR
                *(__attribute__((address_space(3))) T*)(smem + base + OFF_MID + row * ESZ) = CANON_MID ? T(0) + acc : acc;
#else
                *(__attribute__((address_space(3))) T*)(smem + base + pos1[row]) = CANON_MID ? T(0) + acc : acc;
#endif
            };
            constexpr int LAST1 = ROWS1 - 1;
            int row = sub;
            if (row < ROWS1) load1(la, ra, row);
#pragma nounroll
            for (; row < ROWS1; row += 2 * NSUB) {
                const int r2_ = row + NSUB, r3_ = row + 2 * NSUB;
                load1(lb, rb, r2_ < ROWS1 ? r2_ : LAST1);
                sum1(la, ra, row);
                load1(la, ra, r3_ < ROWS1 ? r3_ : LAST1);
                if (r2_ < ROWS1) sum1(lb, rb, r2_);
            }
        }
        __syncthreads();
#endif
#endif
        // ---- list 2: (mid, other operand) -> out; TB terms' operands in flight while the previous TB are summed ----
#if SPLIT > 1
        T part[PASSES2];
#endif
#pragma unroll
        for (int pass = 0; pass < PASSES2; ++pass) {
            const int vrow = sub + pass * NSUB;          // (row, slice)
            if (vrow >= ROWS2 * SPLIT) break;
            const int row = vrow / SPLIT, slice = vrow % SPLIT;
            const u32 oo = oo_reg[pass];
#if (BETA || INIT_SRC) && SPLIT == 1
            T acc = acc0[pass];
#else
            T acc = T(0);                                // (slices start from zero: what the row adds onto joins them at the end)
#endif
#if SORTED
            // tolerance mode, sign-sorted: WPS plus-terms, then WMS minus-terms (both whole batches of TB; the padding multiplies the item's
            // zero element by itself): no sign per term -- two address additions and one fused multiply-add
            {
                T ma[TB], oa[TB], mb[TB], ob[TB];
                auto load2 = [&](T (&mv)[TB], T (&ov)[TB], int q) {      // TB terms from quad q of this (row, slice)
#pragma unroll
                    for (int i = 0; i < TB / 4; ++i) {
#if ENT2_MODE == 3
                        const u32x4 e4 = ((const __attribute__((address_space(3))) u32x4*)(smem + ENT2_AT))[vrow * (WSS / 4) + q + i];
#else
                        const u32x4 e4 = ((const u32x4*)ent2)[vrow * (WSS / 4) + q + i];
#endif
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            mv[4 * i + j] = LDS(base + (e4[j] & 0xffffu));
                            ov[4 * i + j] = LDS(base + (e4[j] >> 16));
                        }
                    }
                };
                constexpr int NBT = WSS / TB, NBP = WPS / TB;            // batches in all, plus-batches first
                auto sum2 = [&](const T (&mv)[TB], const T (&ov)[TB], int b) {
                    if (b < NBP) {
#pragma unroll
                        for (int t = 0; t < TB; ++t) acc = FMA(mv[t], ov[t], acc);
                    } else {
#pragma unroll
                        for (int t = 0; t < TB; ++t) acc = FMA(-mv[t], ov[t], acc);
                    }
                };
                load2(ma, oa, 0);
                int b = 0;
#pragma nounroll
                for (; b + 2 <= NBT; b += 2) {
                    load2(mb, ob, (b + 1) * (TB / 4));
                    sum2(ma, oa, b);
                    load2(ma, oa, (b + 2 < NBT ? b + 2 : NBT - 1) * (TB / 4));
                    sum2(mb, ob, b + 1);
                }
                if (NBT & 1) sum2(ma, oa, NBT - 1);
            }
#else
            constexpr int NB = WS / TB;                  // batches of TB terms
            constexpr int QPT = ENT2_MODE == 2 ? 2 : 4;  // terms per table quad
            const int q0 = slice * (WS / QPT);           // the slice's first quad (WS is a multiple of 4)
#if ENT2_MODE == 2
            T ma[TB], oa[TB], mb[TB], ob[TB];
            u32 sa[TB], sb[TB];
            auto load2 = [&](T (&mv)[TB], T (&ov)[TB], u32 (&sg)[TB], int b) {
#pragma unroll
                for (int q = 0; q < TB / 2; ++q) {
                    const u32x4 e4 = ent2_quad(row, q0 + (TB / 2) * b + q);
                    mv[2 * q] = LDS(base + (e4[0] & 0xffffu));
                    ov[2 * q] = LDS(base + (e4[0] >> 16));
                    sg[2 * q] = e4[1];
                    mv[2 * q + 1] = LDS(base + (e4[2] & 0xffffu));
                    ov[2 * q + 1] = LDS(base + (e4[2] >> 16));
                    sg[2 * q + 1] = e4[3];
                }
            };
            auto sum2 = [&](const T (&mv)[TB], const T (&ov)[TB], const u32 (&sg)[TB]) {
#pragma unroll
                for (int t = 0; t < TB; ++t) {
#if EXACT
                    const T pr_ = mv[t] * ov[t];
                    acc = acc + with_hi(pr_, hi_of(pr_) ^ sg[t]);            // eval.rs:82: (l * r) * (+-1), then +=
#else
                    acc = FMA(with_hi(mv[t], hi_of(mv[t]) ^ sg[t]), ov[t], acc);   // tolerance mode: one rounding per term
#endif
                }
            };
#else
            T ma[TB], oa[TB], sa[TB], mb[TB], ob[TB], sb[TB];
            auto load2 = [&](T (&mv)[TB], T (&ov)[TB], T (&sg)[TB], int b) {
#pragma unroll
                for (int q = 0; q < TB / 4; ++q) {
                    const u32x4 e4 = ent2_quad(row, q0 + (TB / 4) * b + q);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        mv[4 * q + j] = LDS(base + (e4[j] & 0xffffu));
                        ov[4 * q + j] = LDS(base + ((e4[j] >> 16) & 0x7fffu));
                        u32 hi;
                        asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(hi) : "v"(e4[j]), "s"(0x80000000u), "v"(one_hi));   // +-1.0: the high word
                        sg[4 * q + j] = pm_one(hi);
                    }
                }
            };
            auto sum2 = [&](const T (&mv)[TB], const T (&ov)[TB], const T (&sg)[TB]) {
#pragma unroll
                for (int t = 0; t < TB; ++t) acc = FMA(mv[t] * ov[t], sg[t], acc);   // eval.rs:82: the product is rounded, +-1 is exact
            };
#endif
            if (NB > 0) load2(ma, oa, sa, 0);
            int b = 0;
#pragma nounroll
            for (; b + 2 <= NB; b += 2) {
                load2(mb, ob, sb, b + 1);
                sum2(ma, oa, sa);
                load2(ma, oa, sa, b + 2 < NB ? b + 2 : NB - 1);
                sum2(mb, ob, sb);
            }
            if (NB & 1) sum2(ma, oa, sa);
#pragma unroll
            for (int t = NB * TB; t < WS; ++t) {         // the remainder (compile-time count, no padding terms)
#if ENT2_MODE == 2
                const u32x4 e4 = ent2_quad(row, q0 + t / 2);
                const u32 e = e4[2 * (t & 1)], sgb = e4[2 * (t & 1) + 1];
#if EXACT
                const T pr_ = LDS(base + (e & 0xffffu)) * LDS(base + (e >> 16));
                acc = acc + with_hi(pr_, hi_of(pr_) ^ sgb);
#else
                const T m_ = LDS(base + (e & 0xffffu));
                acc = FMA(with_hi(m_, hi_of(m_) ^ sgb), LDS(base + (e >> 16)), acc);
#endif
#else
                const u32 e = ent2_quad(row, q0 + t / 4)[t & 3];
                acc = FMA(LDS(base + (e & 0xffffu)) * LDS(base + ((e >> 16) & 0x7fffu)), pm_one((e & 0x80000000u) | ONE_HI), acc);
#endif
            }
#endif
#if SPLIT > 1
            part[pass] = acc;
#else
            if (it < nitems) out[(item0 + it) * s_out + oo] = acc;
#endif
        }
#if SPLIT > 1
        // the slices of a row meet through LDS (the mid rows are dead by now): partial sums in slice order onto the row's start value
        __syncthreads();
#pragma unroll
        for (int pass = 0; pass < PASSES2; ++pass) {
            const int vrow = sub + pass * NSUB;
            if (vrow < ROWS2 * SPLIT) *(__attribute__((address_space(3))) T*)(smem + base + OFF_MID + vrow * ESZ) = part[pass];
        }
        __syncthreads();
#pragma unroll
        for (int pass = 0; pass < PASSES2; ++pass) {
            const int vrow = sub + pass * NSUB;
            if (vrow < ROWS2 * SPLIT && vrow % SPLIT == 0 && it < nitems) {
#if BETA || INIT_SRC
                T acc = acc0[pass];
#else
                T acc = T(0);
#endif
#pragma unroll
                for (int sl = 0; sl < SPLIT; ++sl) acc = acc + LDS(base + OFF_MID + (vrow + sl) * ESZ);
                out[(item0 + it) * s_out + oo_reg[pass]] = acc;
            }
        }
#endif
        __syncthreads();   // the rows are rewritten by the next group
        if (!more) break;
        g = gn;
        if (pre_next) commit();
        else stage_all(gn * IPB, nnext);
    }
}
)JIT";

std::string chain_source(const Plan& plan, const Step& c, const Step& w, const ChainShape& sh) {
    std::string src;
    auto def = [&](const char* name, int64_t v) { src += std::string("#define ") + name + " " + std::to_string(v) + "\n"; };
    src += plan.dtype == GAAST_F32 ? "typedef float T;\n#define F64 0\n" : "typedef double T;\n#define F64 1\n";
    def("ESZ", sh.esz); def("NT", sh.threads); def("IPB", sh.ipb); def("NSUB", sh.threads / sh.ipb); def("STRIDE_B", sh.stride * sh.esz);
    def("L1", sh.l1); def("R1", sh.r1); def("R2", sh.alias ? 0 : sh.r2); def("MID", sh.mid); def("NEGLEN", sh.neg_len); def("NEG_IS_LEFT", sh.neg_is_left ? 1 : 0);
    def("OFF_L1", sh.off_l1 * sh.esz); def("OFF_R1", sh.off_r1 * sh.esz); def("OFF_NEG", sh.off_neg * sh.esz); def("OFF_MID", sh.off_mid * sh.esz);
    def("OFF_R2", (sh.alias ? 0 : sh.off_r2) * sh.esz); def("HAS_R2", sh.alias ? 0 : 1);
    def("ROWS1", sh.rows1); def("W1", sh.w1); def("W1S", sh.w1s); def("ROWS2", sh.rows2); def("W2", sh.w2); def("W2P", sh.w2p);
    def("CANON_L1", w.canon_a); def("CANON_R1", w.canon_b); def("CANON_R2", sh.side == 1 ? c.canon_b : c.canon_a);
    def("CANON_MID", sh.side == 1 ? c.canon_a : c.canon_b); def("COVERED", sh.covered ? 1 : 0); def("BETA", sh.has_init ? 0 : c.beta);
    def("SINGLE", sh.single ? 1 : 0); def("INIT_SRC", sh.has_init ? 1 : 0);
    bool pos1_linear = true;   // row k of list 1 is component k of the mid row (the usual case): no table, no load
    for (int64_t row = 0; row < sh.rows1; ++row) pos1_linear = pos1_linear && int64_t(w.list.row_out[size_t(row)]) == row;
    def("POS1_LINEAR", pos1_linear ? 1 : 0);
    // EXACT: every product rounded, then added (eval.rs:82), rows summed whole -- the reference's bits.  Otherwise (the default,
    // the dense products' tolerance contract): rows of list 2 in slices, and l * r + acc as one fused multiply-add
    def("EXACT", (plan.flags & GAAST_FLAG_EXACT_ORDER) ? 1 : 0);
    def("XREG", sh.xreg ? 1 : 0);
    def("SORTED", sh.sorted ? 1 : 0); def("WPS", sh.wps); def("WMS", sh.wms); def("WSS", sh.wss); def("OFF_ZERO", sh.off_zero * sh.esz);
    def("SPLIT", sh.split); def("WS", sh.w2 / sh.split);                    // slices per row of list 2, terms per slice
    def("PASSES2", (sh.rows2 * sh.split + sh.threads / sh.ipb - 1) / (sh.threads / sh.ipb));   // (row, slice) pairs of list 2 per thread
    // terms of list 2 in flight per register set: the registers of two waves per SIMD (512 threads) hold 8 f64 / 16 f32 terms twice; more
    // threads (a single list with many rows x items), fewer registers each
    def("TB", (plan.dtype == GAAST_F32 ? 16 : 8) / (sh.threads > 512 ? 2 : 1));
    def("ENT2_MODE", sh.ent2_mode); def("ENT1_MODE", sh.ent1_mode); def("ENT2_AT", sh.ent2_at); def("ENT1_AT", sh.ent1_at); def("SMEM_BYTES", sh.used);
    return src + kChainKernel;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// The list chain specialised per program (round 4; the generic k_product_ell_chain is the fallback when hiprtc is not
// available).  What the generic kernel paid for: run-time widths and lengths, a row-per-lane first list whose 64 lanes gather
// 64 different offsets of ONE item (bank conflicts: 39 % of the LDS cycles), nine vector instructions per term.  Here:
//   * lane = (row, item) in BOTH lists, the IPB items of the workgroup fastest: the lanes of one LDS access group read the
//     SAME offset of different items, item stride odd (in elements) -> no bank conflict at IPB = 32;
//   * an entry is one word of byte offsets from the ITEM's base: list 1 [15:0] left | [31:16] right, the sign folded into
//     the choice between the smaller operand's image and its NEGATED image (l * (-r) = -(l * r) exactly: eval.rs:82 with
//     coeff = -1); list 2 [15:0] mid | [30:16] other | [31] sign, applied as fma(l * r, +-1.0, acc): the product is rounded
//     first, +-1 is exact, the sum is rounded once -- the reference's three roundings;
//   * entries are read from global memory (the tables are shared by every workgroup and stay in L2 / L1), a quad of entries
//     per 16-byte load, the next quads in flight while the current ones are used; no run-time width, no padding terms
//     (acc + (+0.0) would turn a -0.0 accumulator of a beta = 1 list into +0.0);
//   * reference order and roundings: bit-identical to the two-launch plan and to the oracle.
// ---------------------------------------------------------------------------------------------------------------------
// wp == nullptr: a SINGLE list with few long rows (rows2 x IPB lanes instead of rows2; k_product_ell gives a row to a thread): the
// left operand plays the staged "mid" row (l1 = r1 = 0, mid = its length), the right one is list 2's own operand r2 (alias 0,
// side 1).  init_off (single list only): acc starts from 0.0 + init[row's offset] -- a covering copy_grades_from of an input
// folded into the list that accumulates onto it ((a + b * c).g(2): one launch).
void make_chain_jit(const Plan& plan, Step& c, const Step* wp, int64_t l1, int64_t r1, int64_t mid, int64_t r2, int alias, int side, bool covered,
                    const std::vector<uint32_t>* init_off) {
    if (plan.flags & (GAAST_FLAG_NO_JIT | GAAST_FLAG_DEBUG_JIT_FAILS)) return;
    static const Step no_list;
    const Step& w = wp ? *wp : no_list;
    ChainShape sh;
    if (!chain_tables(plan, c, w, wp == nullptr, l1, r1, mid, r2, alias, side, covered, init_off, sh)) return;
    c.cj.on = 1;
    c.cj.source = chain_source(plan, c, w, sh);
    const int64_t lay[7] = {sh.off_l1, sh.off_r1, sh.off_neg, sh.off_mid, sh.alias ? -1 : sh.off_r2, sh.stride, sh.neg_is_left ? 1 : 0};
    for (int i = 0; i < 7; ++i) c.cj.layout[i] = int(lay[i]);
    c.cj.fmt[0] = int(sh.w1s);
    c.cj.fmt[1] = sh.ent2_mode;
    c.cj.sorted[0] = int(sh.wps);
    c.cj.sorted[1] = int(sh.wms);
    c.cj.sorted[2] = int(sh.off_zero * sh.esz);
    c.cj.xreg = sh.xreg ? 1 : 0;
    c.cj.split = int(sh.split);
    c.cj.ipb = int(sh.ipb);
    c.cj.threads = int(sh.threads);
    c.cj.lds = size_t(sh.used);
}

}  // namespace gaast
