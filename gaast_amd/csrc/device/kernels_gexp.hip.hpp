// kernels_gexp.hip.hpp -- the general multivector exponential and its reverse mode (GAAST_OP_GEXP / GAAST_OP_GEXP_ADJ, gaast_hip.h;
// Step::GEXP / Step::GEXP_ADJ; no reference counterpart)
//
//   k_mv_gexp<T, N>       res += exp(A) over a blade set S of N = 2, 4, ... 64 blades (every blade, or the even ones)
//   k_mv_gexp_adj<T, N>   res += the cotangent of A, from A and the cotangent g of exp(A)
//
// Scaling and squaring on the left-multiplication matrix L[r][j] = coeff(r, j) A[r xor j] of k_mv_inverse (plan.hpp: Step::Inverse,
// the same blade order and tables).  Per item, as gaast_hip.h states it:
//   theta = wmax * sum |A_a| (a butterfly over the item's lanes);  s = the least integer >= 0 with theta 2^-s <= 1/2;  A_s = A 2^-s;
//   q_M = e_0,  q_(k-1) = e_0 + (A_s q_k) / k  for k = M ... 1  (M = 8 in f32, 14 in f64);   Y_0 = q_0,  Y_(i+1) = Y_i Y_i  for i < s.
// theta not finite or > 2048 (s > 12) is a domain error: the forward stores quiet NaNs and counts the item in *dom.
//
// Lane layout (both kernels): k_mv_inverse's.  N consecutive lanes own one item, lane r the component of blade S[r]; 64 / N items per
// wave, four waves per workgroup, workgroups stride over the groups of 256 / N items.  Every product is P[r] = sum_j L_X[r][j] Z[j]
// with j ascending, lane r gathering X[r xor j] (a permutation of the item's N consecutive LDS words: conflict-free) and Z[j] (one
// address per item: a broadcast), the coefficient rebuilt from a sign word per row and the metric factor table in LDS.
//   k_mv_gexp      Lane r holds row r of L_(A_s) in N registers through the Horner phase (gathered once, as k_mv_inverse gathers its
//                  row; the coefficients are kept out of registers the same way), q ping-pongs between two LDS rows: one barrier
//                  per Horner step.  A squaring gathers row r of L_Y from the LDS copy of Y.  s differs per item: the squaring loop
//                  runs to the largest s of the workgroup's items and an item keeps its Y by a select once i >= s, so the barriers
//                  stay uniform and nothing exits early.
//   k_mv_gexp_adj  recomputes the forward, everything gathered from LDS, keeping q_0 ... q_M of its component in registers (static
//                  indices: the loops over k unroll) and Y_0 ... Y_s in LDS (13 x 256 values), then runs the reverse sweep
//                      g <- ADJL(g, Y_i) + ADJR(g, Y_i)  for i = s-1 ... 0;
//                      for k = 1 ... M:  h = g / k;  dA_s += ADJL(h, q_k);  g <- ADJR(h, A_s);      dA = 2^-s dA_s
//                  with ADJL(g, Z)[a] = sum_b coeff(a, b) Z[b] g[a xor b], ADJR(g, X)[b] = sum_a coeff(a, b) X[a] g[a xor b] (the sign
//                  words of both are built on the host; the metric factor of either is weight[S[a] & S[b]]).  No domain check: a
//                  domain-error item scales by NaN, so every component of its cotangent is NaN by arithmetic.
//   k_mv_gexp_jvp<T, N>   res += the Frechet derivative of exp at A in direction h (GAAST_OP_GEXP_JVP; Step::GEXP_JVP)
//   k_mv_gexp_adj2<T, N>  res += the gradient in A of <g, that derivative> (GAAST_OP_GEXP_ADJ2; Step::GEXP_ADJ2)
// The second-order pair, in k_mv_gexp_adj's layout, s from A alone, h_s = 2^-s h, everything gathered from LDS:
//   k_mv_gexp_jvp  a pure forward with no stored history.  A_s and h_s stay in LDS; (q, qd) ping-pong between two LDS rows each
//                  through the Horner steps qd_(k-1) = (h_s q_k + A_s qd_k) / k (three products with the value's; qd_M = 0: two
//                  at k = M), then (Y, Yd) through the squarings Yd_(i+1) = Yd_i Y_i + Y_i Yd_i (three products).
//                  Static LDS: 6 rows of 256 T (A_s, h_s; q, qd twice each) + the 128 weights + 4 ints = (6 * 256 + 128) sizeof(T) + 16.
//   k_mv_gexp_adj2 recomputes that forward pair keeping q_0 ... q_M and qd_0 ... qd_M of its component in registers (2 (M + 1)
//                  values, static indices) and Y_0 ... Y_s, Yd_0 ... Yd_s in LDS (2 x 13 rows), then sweeps with the cotangent pair
//                  (G of the values, Gd of the tangents; Gd = g, G = 0):
//                      G <- ((ADJL(G, Y_i) + ADJR(G, Y_i)) + ADJR(Gd, Yd_i)) + ADJL(Gd, Yd_i);  Gd <- ADJL(Gd, Y_i) + ADJR(Gd, Y_i)
//                      for k = 1 ... M:  w = G / k, wd = Gd / k;  dA_s += ADJL(w, q_k) + ADJL(wd, qd_k);
//                                        G <- ADJR(w, A_s) + ADJR(wd, h_s);  Gd <- ADJR(wd, A_s);             dA = 2^-s dA_s
//                  six adjoint rows per squaring, five per Horner step.
//                  Static LDS: 36 rows of 256 T (A_s, h_s; q, qd, G, Gd twice each; 13 Y, 13 Yd) + the 128 weights + 4 ints
//                  = (36 * 256 + 128) sizeof(T) + 16: 37392 bytes in f32, 74768 in f64 -- above 64 KiB, which gfx950 allows a
//                  workgroup (160 KiB per CU), and two workgroups still share a CU.
//                  Neither kernel checks a domain or counts: a domain-error item scales A and h by NaN.
// Offsets in int64_t; any row stride (0: one operand shared by every item), padding or alignment takes the same scalar accesses.
#pragma once
#include "kernels_inverse.hip.hpp"

namespace gaast {

template <typename T>
struct GexpArgs {
    T* res;
    const T* in;
    const T* cot;             // k_mv_gexp_adj: the cotangent rows
    int64_t res_stride, in_stride, cot_stride, batch;
    const int32_t* a_off;     // [N] operand offset of blade j, -1 = absent
    const int32_t* res_off;   // [N] result offset of blade j, -1 = not produced
    const int32_t* g_off;     // [N] cotangent offset of blade j, -1 = absent (k_mv_gexp_adj)
    const uint64_t* neg;      // [N] row r: bit j = the reordering sign of L[r][j] is minus
    const uint64_t* neg_l;    // [N] ADJL's sign words (k_mv_gexp_adj)
    const uint64_t* neg_r;    // [N] ADJR's sign words (k_mv_gexp_adj)
    const T* weight;          // [1 << n] metric factor by shared-vector set
    uint64_t a_neg;           // bit j: operand component j is negated
    T wmax;                   // the largest |weight|
    int n;                    // dimension of the algebra
    int even;                 // S is the even blades
    int beta;                 // 0: the zero fill of a fresh result is folded in
    unsigned long long* dom;
};

namespace gexp_detail {

using namespace inverse_detail;

template <typename T>
constexpr int taylor_degree() { return sizeof(T) == 4 ? 8 : 14; }   // the least m with (1/2)^(m+1) / (m+1)! <= eps / 2
constexpr int kMaxSquarings = 12;

__device__ __forceinline__ float frexp_m(float x, int* e) { return __builtin_frexpf(x, e); }
__device__ __forceinline__ double frexp_m(double x, int* e) { return __builtin_frexp(x, e); }
__device__ __forceinline__ float ldexp_m(float x, int e) { return __builtin_ldexpf(x, e); }
__device__ __forceinline__ double ldexp_m(double x, int e) { return __builtin_ldexp(x, e); }

// theta of my item (every lane of the item gets the same bits: a + b is commutative), and from it the number of squarings
template <typename T, int N>
__device__ __forceinline__ int squarings_of(T v, T wmax, bool* bad) {
    T th = abs_m(v);
#pragma unroll
    for (int m = N / 2; m >= 1; m >>= 1) th = th + __shfl_xor(th, m);
    th = th * wmax;
    *bad = !(th <= T(2048));                       // (a NaN or an infinite theta fails the comparison too)
    int s = 0;
    if (!*bad && th > T(0.5)) {
        int e;
        const T f = frexp_m(th, &e);               // theta = f 2^e, 1/2 <= f < 1
        s = e + int(f != T(0.5));
    }
    return s;
}

// the largest s over the workgroup (every lane of a wave ends with its wave's)
__device__ __forceinline__ int wave_max(int s) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s = max(s, __shfl_xor(s, m));
    return s;
}

// P[r] = sum_j L_X[r][j] Z[j], j ascending: the metric factor's index is S[j] & ~S[r] = ((j & ~r) << e) | (e & parity(j) & ~parity(r))
template <typename T, int N>
__device__ __forceinline__ T product_row(const T* X, const T* Z, const T* weight, uint32_t r, uint64_t neg, uint32_t e) {
    const uint32_t npar = e & ~uint32_t(__builtin_popcount(r)) & 1u;
    constexpr int UNROLL = N <= 8 ? 1 : 8;   // (a sum that unrolls fully at every one of its uses costs k_mv_gexp_adj hundreds of registers)
    T acc = T(0);
#pragma unroll UNROLL
    for (uint32_t j = 0; j < uint32_t(N); ++j) {
        const uint32_t idx = ((j & ~r) << e) | (uint32_t(__builtin_popcount(j)) & npar);
        const T c = flip_sign(weight[idx] * X[r ^ j], uint32_t(neg >> j) & 1u);
        acc = fma_m(c, Z[j], acc);
    }
    return acc;
}

// ADJL(G, V)[c] with sgn = neg_l[c], ADJR(G, V)[c] with sgn = neg_r[c]: sum_t +-weight[S[c] & S[t]] V[t] G[c xor t], t ascending
template <typename T, int N>
__device__ __forceinline__ T adjoint_row(const T* V, const T* G, const T* weight, uint32_t c, uint64_t sgn, uint32_t e) {
    const uint32_t par = e & uint32_t(__builtin_popcount(c)) & 1u;
    constexpr int UNROLL = N <= 8 ? 1 : 8;
    T acc = T(0);
#pragma unroll UNROLL
    for (uint32_t t = 0; t < uint32_t(N); ++t) {
        const uint32_t idx = ((c & t) << e) | (uint32_t(__builtin_popcount(t)) & par);
        const T u = flip_sign(weight[idx] * V[t], uint32_t(sgn >> t) & 1u);
        acc = fma_m(u, G[c ^ t], acc);
    }
    return acc;
}

}  // namespace gexp_detail

template <typename T, int N>
__global__ __launch_bounds__(256, 2) void k_mv_gexp(const GexpArgs<T> p) {
    using namespace gexp_detail;
    static_assert(N == 2 || N == 4 || N == 8 || N == 16 || N == 32 || N == 64, "one item per N lanes of a wave");
    constexpr int IPB = 256 / N;                 // items of a workgroup
    constexpr int M = taylor_degree<T>();
    __shared__ T arow[256];                      // [IPB][N]: an item's scaled operand A_s by blade index
    __shared__ T qrow[2][256];                   // q of the Horner steps, then Y of the squarings: read from one, written to the other
    __shared__ T weight[128];
    __shared__ int wave_s[4];
    const int tid = int(threadIdx.x);
    const int r = tid & (N - 1), g = tid / N;    // my row of the item, my item of the workgroup
    if (tid < (1 << p.n)) weight[tid] = p.weight[tid];
    const int32_t a_off = p.a_off[r], res_off = p.res_off[r];
    const bool a_neg = ((p.a_neg >> r) & 1ULL) != 0;
    const uint64_t neg = p.neg[r];
    const uint32_t e = uint32_t(p.even);
    const T e0 = r == 0 ? T(1) : T(0);
    const T* const mine_a = arow + g * N;
    for (int64_t base = int64_t(blockIdx.x) * IPB; base < p.batch; base += int64_t(gridDim.x) * IPB) {
        const int64_t item = base + g;
        const bool live = item < p.batch;
        T v = T(0);
        if (live && a_off >= 0) v = p.in[item * p.in_stride + a_off];
        if (a_neg) v = -v;
        bool bad;
        const int s = squarings_of<T, N>(v, p.wmax, &bad);   // (a domain error: s = 0, the arithmetic runs on whatever values it has)
        const int ws = wave_max(s);
        __syncthreads();                         // (the previous group's rows have been read; the first pass: `weight` is written)
        arow[tid] = v * ldexp_m(T(1), -s);
        qrow[0][tid] = e0;                       // q_M
        if ((tid & 63) == 0) wave_s[tid >> 6] = ws;
        __syncthreads();
        // my row of L_(A_s), as k_mv_inverse builds its row: ~r and the sign word are made opaque per pass, else the compiler keeps
        // the N coefficients in N more registers than the row itself
        uint32_t nr = ~uint32_t(r);
        uint32_t neg_lo = uint32_t(neg), neg_hi = uint32_t(neg >> 32);
        asm volatile("" : "+v"(nr), "+v"(neg_lo), "+v"(neg_hi));
        const uint32_t npar = e & ~uint32_t(__builtin_popcount(~nr)) & 1u;   // e & ~parity(r)
        T row[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const uint32_t idx = ((uint32_t(j) & nr) << e) | ((uint32_t(__builtin_popcount(uint32_t(j))) & 1u) ? npar : 0u);
            const T c = weight[idx] * mine_a[(~nr & uint32_t(N - 1)) ^ uint32_t(j)];
            row[j] = flip_sign(c, ((j < 32 ? neg_lo : neg_hi) >> (j & 31)) & 1u);
            if ((j & 7) == 7) __builtin_amdgcn_sched_barrier(0);   // (else all 2 N loads of the gather are in flight at once, each in a register)
        }
        T y = e0;
#pragma unroll
        for (int k = M; k >= 1; --k) {           // q_(k-1) = e_0 + (A_s q_k) / k
            const T* const q = qrow[(M - k) & 1] + g * N;
            T acc = T(0);
#pragma unroll
            for (int j = 0; j < N; ++j) acc = fma_m(row[j], q[j], acc);
            y = e0 + acc / T(k);
            qrow[(M - k + 1) & 1][tid] = y;
            __syncthreads();
        }
        int cur = M & 1;                         // Y_0 = q_0 sits in qrow[cur]
        const int smax = max(max(wave_s[0], wave_s[1]), max(wave_s[2], wave_s[3]));
        for (int i = 0; i < smax; ++i) {         // Y_(i+1) = Y_i Y_i while i < s
            const T* const Y = qrow[cur] + g * N;
            const T sq = product_row<T, N>(Y, Y, weight, ~nr, neg, e);   // (~nr: r, opaque like the row's)
            y = i < s ? sq : y;
            cur ^= 1;
            qrow[cur][tid] = y;
            __syncthreads();
        }
        if (live) {
            if (res_off >= 0) {
                T* d = p.res + item * p.res_stride + res_off;
                *d = bad ? qnan(T(0)) : (p.beta ? *d : T(0)) + y;
            }
            if (bad && r == 0) atomicAdd(p.dom, 1ull);
        }
    }
}

template <typename T, int N>
__global__ __launch_bounds__(256) void k_mv_gexp_adj(const GexpArgs<T> p) {
    using namespace gexp_detail;
    static_assert(N == 2 || N == 4 || N == 8 || N == 16 || N == 32 || N == 64, "one item per N lanes of a wave");
    constexpr int IPB = 256 / N;
    constexpr int M = taylor_degree<T>();
    __shared__ T arow[256];                          // A_s
    __shared__ T qrow[2][256];                       // the forward's q, then q_k of the sweep
    __shared__ T grow[2][256];                       // the running cotangent (h = g / k in the Horner part of the sweep)
    __shared__ T yrow[kMaxSquarings + 1][256];       // Y_0 ... Y_s
    __shared__ T weight[128];
    __shared__ int wave_s[4];
    const int tid = int(threadIdx.x);
    const int r = tid & (N - 1), g = tid / N;
    if (tid < (1 << p.n)) weight[tid] = p.weight[tid];
    const int32_t a_off = p.a_off[r], res_off = p.res_off[r], g_off = p.g_off[r];
    const bool a_neg = ((p.a_neg >> r) & 1ULL) != 0;
    const uint64_t neg = p.neg[r], neg_l = p.neg_l[r], neg_r = p.neg_r[r];
    const uint32_t e = uint32_t(p.even);
    const T e0 = r == 0 ? T(1) : T(0);
    const int it0 = g * N;                           // my item's words of a row
    for (int64_t base = int64_t(blockIdx.x) * IPB; base < p.batch; base += int64_t(gridDim.x) * IPB) {
        // r is made opaque per pass (an empty asm statement, no instruction): no coefficient depends on the item, so where the sums
        // unroll fully (N <= 8) the compiler would keep the coefficients of every step of both sweeps in registers across items
        uint32_t ur = uint32_t(r);
        asm volatile("" : "+v"(ur));
        const int64_t item = base + g;
        const bool live = item < p.batch;
        T v = T(0), gv = T(0);
        if (live && a_off >= 0) v = p.in[item * p.in_stride + a_off];
        if (live && g_off >= 0) gv = p.cot[item * p.cot_stride + g_off];
        if (a_neg) v = -v;
        bool bad;
        const int s = squarings_of<T, N>(v, p.wmax, &bad);
        const T scale = bad ? qnan(T(0)) : ldexp_m(T(1), -s);
        const int ws = wave_max(s);
        __syncthreads();                             // (the previous group's rows have been read; the first pass: `weight` is written)
        arow[tid] = v * scale;
        qrow[0][tid] = e0;                           // q_M
        if ((tid & 63) == 0) wave_s[tid >> 6] = ws;
        __syncthreads();
        // the forward again, keeping every q_k of my component
        T q[M + 1];
        q[M] = e0;
#pragma unroll
        for (int k = M; k >= 1; --k) {
            q[k - 1] = e0 + product_row<T, N>(arow + it0, qrow[(M - k) & 1] + it0, weight, ur, neg, e) / T(k);
            qrow[(M - k + 1) & 1][tid] = q[k - 1];
            if (k == 1) {
                yrow[0][tid] = q[0];                 // Y_0
                grow[0][tid] = gv;                   // the sweep starts from g
            }
            __syncthreads();
        }
        const int smax = max(max(wave_s[0], wave_s[1]), max(wave_s[2], wave_s[3]));
        T y = q[0];
        for (int i = 0; i < smax; ++i) {             // (smax <= 12: yrow[i + 1] exists)
            const T sq = product_row<T, N>(yrow[i] + it0, yrow[i] + it0, weight, ur, neg, e);
            y = i < s ? sq : y;
            yrow[i + 1][tid] = y;
            __syncthreads();
        }
        // the reverse sweep.  Squarings: g <- ADJL(g, Y_i) + ADJR(g, Y_i), i = s-1 ... 0
        int cur = 0;
        T gc = gv;
        for (int i = smax - 1; i >= 0; --i) {
            const T l = adjoint_row<T, N>(yrow[i] + it0, grow[cur] + it0, weight, ur, neg_l, e);
            const T rr = adjoint_row<T, N>(yrow[i] + it0, grow[cur] + it0, weight, ur, neg_r, e);
            gc = i < s ? l + rr : gc;
            cur ^= 1;
            grow[cur][tid] = gc;
            __syncthreads();
        }
        // Horner: h = g / k; dA_s += ADJL(h, q_k); g <- ADJR(h, A_s).  grow[cur] holds h (k = 1: g itself), qrow[k & 1] holds q_k
        qrow[1][tid] = q[1];
        __syncthreads();
        T da = T(0);
#pragma unroll
        for (int k = 1; k <= M; ++k) {
            da = da + adjoint_row<T, N>(qrow[k & 1] + it0, grow[cur] + it0, weight, ur, neg_l, e);
            if (k < M) {
                const T gn = adjoint_row<T, N>(arow + it0, grow[cur] + it0, weight, ur, neg_r, e);
                cur ^= 1;
                grow[cur][tid] = gn / T(k + 1);
                qrow[(k + 1) & 1][tid] = q[k + 1];
                __syncthreads();
            }
        }
        if (live && res_off >= 0) {
            T* d = p.res + item * p.res_stride + res_off;
            *d = (p.beta ? *d : T(0)) + da * scale;
        }
    }
}

// ---- second order: GAAST_OP_GEXP_JVP / GAAST_OP_GEXP_ADJ2 ------------------------------------------------------------------------
template <typename T>
struct Gexp2Args {
    T* res;
    const T* in;              // the forward operand A
    const T* cot;             // g (k_mv_gexp_adj2)
    const T* tan;             // h
    int64_t res_stride, in_stride, cot_stride, tan_stride, batch;
    const int32_t* a_off;     // [N] operand offset of blade j, -1 = absent
    const int32_t* res_off;   // [N] result offset of blade j, -1 = not produced
    const int32_t* g_off;     // [N] offset of blade j in g's row, -1 = absent (k_mv_gexp_adj2)
    const int32_t* h_off;     // [N] offset of blade j in h's row, -1 = absent
    const uint64_t* neg;      // [N] the sign words of L
    const uint64_t* neg_l;    // [N] ADJL's (k_mv_gexp_adj2)
    const uint64_t* neg_r;    // [N] ADJR's (k_mv_gexp_adj2)
    const T* weight;          // [1 << n] metric factor by shared-vector set
    uint64_t a_neg;           // bit j: operand component j is negated
    T wmax;
    int n;
    int even;
    int beta;                 // 0: the zero fill of a fresh result is folded in
};

template <typename T, int N>
__global__ __launch_bounds__(256) void k_mv_gexp_jvp(const Gexp2Args<T> p) {
    using namespace gexp_detail;
    static_assert(N == 2 || N == 4 || N == 8 || N == 16 || N == 32 || N == 64, "one item per N lanes of a wave");
    constexpr int IPB = 256 / N;
    constexpr int M = taylor_degree<T>();
    __shared__ T arow[256];                          // A_s
    __shared__ T hrow[256];                          // h_s
    __shared__ T qrow[2][256];                       // q of the Horner steps, then Y of the squarings
    __shared__ T drow[2][256];                       // qd, then Yd
    __shared__ T weight[128];
    __shared__ int wave_s[4];
    const int tid = int(threadIdx.x);
    const int r = tid & (N - 1), g = tid / N;
    if (tid < (1 << p.n)) weight[tid] = p.weight[tid];
    const int32_t a_off = p.a_off[r], res_off = p.res_off[r], h_off = p.h_off[r];
    const bool a_neg = ((p.a_neg >> r) & 1ULL) != 0;
    const uint64_t neg = p.neg[r];
    const uint32_t e = uint32_t(p.even);
    const T e0 = r == 0 ? T(1) : T(0);
    const int it0 = g * N;
    for (int64_t base = int64_t(blockIdx.x) * IPB; base < p.batch; base += int64_t(gridDim.x) * IPB) {
        uint32_t ur = uint32_t(r);                   // (opaque per pass, as in k_mv_gexp_adj)
        asm volatile("" : "+v"(ur));
        const int64_t item = base + g;
        const bool live = item < p.batch;
        T v = T(0), hv = T(0);
        if (live && a_off >= 0) v = p.in[item * p.in_stride + a_off];
        if (live && h_off >= 0) hv = p.tan[item * p.tan_stride + h_off];
        if (a_neg) v = -v;
        bool bad;
        const int s = squarings_of<T, N>(v, p.wmax, &bad);
        const T scale = bad ? qnan(T(0)) : ldexp_m(T(1), -s);
        const int ws = wave_max(s);
        __syncthreads();                             // (the previous group's rows have been read; the first pass: `weight` is written)
        arow[tid] = v * scale;
        hrow[tid] = hv * scale;
        qrow[0][tid] = e0;                           // q_M
        drow[0][tid] = T(0);                         // qd_M
        if ((tid & 63) == 0) wave_s[tid >> 6] = ws;
        __syncthreads();
        T y = e0, yd = T(0);
#pragma unroll
        for (int k = M; k >= 1; --k) {               // q_(k-1) = e_0 + (A_s q_k) / k;  qd_(k-1) = (h_s q_k + A_s qd_k) / k
            const T* const q = qrow[(M - k) & 1] + it0;
            const T* const qd = drow[(M - k) & 1] + it0;
            const T aq = product_row<T, N>(arow + it0, q, weight, ur, neg, e);
            const T hq = product_row<T, N>(hrow + it0, q, weight, ur, neg, e);
            const T ad = k < M ? product_row<T, N>(arow + it0, qd, weight, ur, neg, e) : T(0);   // (qd_M = 0)
            y = e0 + aq / T(k);
            yd = (hq + ad) / T(k);
            qrow[(M - k + 1) & 1][tid] = y;
            drow[(M - k + 1) & 1][tid] = yd;
            __syncthreads();
        }
        int cur = M & 1;                             // (Y_0, Yd_0) sit in qrow[cur], drow[cur]
        const int smax = max(max(wave_s[0], wave_s[1]), max(wave_s[2], wave_s[3]));
        for (int i = 0; i < smax; ++i) {             // Yd_(i+1) = Yd_i Y_i + Y_i Yd_i,  Y_(i+1) = Y_i Y_i  while i < s
            const T* const Y = qrow[cur] + it0;
            const T* const Yd = drow[cur] + it0;
            const T sq = product_row<T, N>(Y, Y, weight, ur, neg, e);
            const T dl = product_row<T, N>(Yd, Y, weight, ur, neg, e);
            const T dr = product_row<T, N>(Y, Yd, weight, ur, neg, e);
            y = i < s ? sq : y;
            yd = i < s ? dl + dr : yd;
            cur ^= 1;
            qrow[cur][tid] = y;
            drow[cur][tid] = yd;
            __syncthreads();
        }
        if (live && res_off >= 0) {
            T* d = p.res + item * p.res_stride + res_off;
            *d = (p.beta ? *d : T(0)) + yd;
        }
    }
}

template <typename T, int N>
__global__ __launch_bounds__(256) void k_mv_gexp_adj2(const Gexp2Args<T> p) {
    using namespace gexp_detail;
    static_assert(N == 2 || N == 4 || N == 8 || N == 16 || N == 32 || N == 64, "one item per N lanes of a wave");
    constexpr int IPB = 256 / N;
    constexpr int M = taylor_degree<T>();
    __shared__ T arow[256];                          // A_s
    __shared__ T hrow[256];                          // h_s
    __shared__ T qrow[2][256];                       // the forward's q, then q_k of the sweep
    __shared__ T drow[2][256];                       // the forward's qd, then qd_k of the sweep
    __shared__ T grow[2][256];                       // G (w = G / k in the Horner part of the sweep)
    __shared__ T gdrow[2][256];                      // Gd (wd)
    __shared__ T yrow[kMaxSquarings + 1][256];       // Y_0 ... Y_s
    __shared__ T ydrow[kMaxSquarings + 1][256];      // Yd_0 ... Yd_s
    __shared__ T weight[128];
    __shared__ int wave_s[4];
    const int tid = int(threadIdx.x);
    const int r = tid & (N - 1), g = tid / N;
    if (tid < (1 << p.n)) weight[tid] = p.weight[tid];
    const int32_t a_off = p.a_off[r], res_off = p.res_off[r], g_off = p.g_off[r], h_off = p.h_off[r];
    const bool a_neg = ((p.a_neg >> r) & 1ULL) != 0;
    const uint64_t neg = p.neg[r], neg_l = p.neg_l[r], neg_r = p.neg_r[r];
    const uint32_t e = uint32_t(p.even);
    const T e0 = r == 0 ? T(1) : T(0);
    const int it0 = g * N;
    for (int64_t base = int64_t(blockIdx.x) * IPB; base < p.batch; base += int64_t(gridDim.x) * IPB) {
        uint32_t ur = uint32_t(r);                   // (opaque per pass, as in k_mv_gexp_adj)
        asm volatile("" : "+v"(ur));
        const int64_t item = base + g;
        const bool live = item < p.batch;
        T v = T(0), gv = T(0), hv = T(0);
        if (live && a_off >= 0) v = p.in[item * p.in_stride + a_off];
        if (live && g_off >= 0) gv = p.cot[item * p.cot_stride + g_off];
        if (live && h_off >= 0) hv = p.tan[item * p.tan_stride + h_off];
        if (a_neg) v = -v;
        bool bad;
        const int s = squarings_of<T, N>(v, p.wmax, &bad);
        const T scale = bad ? qnan(T(0)) : ldexp_m(T(1), -s);
        const int ws = wave_max(s);
        __syncthreads();                             // (the previous group's rows have been read; the first pass: `weight` is written)
        arow[tid] = v * scale;
        hrow[tid] = hv * scale;
        qrow[0][tid] = e0;                           // q_M
        drow[0][tid] = T(0);                         // qd_M
        if ((tid & 63) == 0) wave_s[tid >> 6] = ws;
        __syncthreads();
        // the forward pair again, keeping every q_k and qd_k of my component
        T q[M + 1], qd[M + 1];
        q[M] = e0;
        qd[M] = T(0);
#pragma unroll
        for (int k = M; k >= 1; --k) {
            const T* const qk = qrow[(M - k) & 1] + it0;
            const T aq = product_row<T, N>(arow + it0, qk, weight, ur, neg, e);
            const T hq = product_row<T, N>(hrow + it0, qk, weight, ur, neg, e);
            const T ad = k < M ? product_row<T, N>(arow + it0, drow[(M - k) & 1] + it0, weight, ur, neg, e) : T(0);   // (qd_M = 0)
            q[k - 1] = e0 + aq / T(k);
            qd[k - 1] = (hq + ad) / T(k);
            qrow[(M - k + 1) & 1][tid] = q[k - 1];
            drow[(M - k + 1) & 1][tid] = qd[k - 1];
            if (k == 1) {
                yrow[0][tid] = q[0];                 // Y_0, Yd_0
                ydrow[0][tid] = qd[0];
                grow[0][tid] = T(0);                 // the sweep starts from G = 0, Gd = g
                gdrow[0][tid] = gv;
            }
            __syncthreads();
        }
        const int smax = max(max(wave_s[0], wave_s[1]), max(wave_s[2], wave_s[3]));
        T y = q[0], yd = qd[0];
        for (int i = 0; i < smax; ++i) {             // (smax <= 12: row i + 1 exists)
            const T* const Y = yrow[i] + it0;
            const T* const Yd = ydrow[i] + it0;
            const T sq = product_row<T, N>(Y, Y, weight, ur, neg, e);
            const T dl = product_row<T, N>(Yd, Y, weight, ur, neg, e);
            const T dr = product_row<T, N>(Y, Yd, weight, ur, neg, e);
            y = i < s ? sq : y;
            yd = i < s ? dl + dr : yd;
            yrow[i + 1][tid] = y;
            ydrow[i + 1][tid] = yd;
            __syncthreads();
        }
        // the sweep.  Squarings, i = s-1 ... 0, both members from the old pair
        int cur = 0;
        T gc = T(0), gdc = gv;
        for (int i = smax - 1; i >= 0; --i) {
            const T* const Y = yrow[i] + it0;
            const T* const Yd = ydrow[i] + it0;
            const T* const G = grow[cur] + it0;
            const T* const Gd = gdrow[cur] + it0;
            const T t1 = adjoint_row<T, N>(Y, G, weight, ur, neg_l, e);
            const T t2 = adjoint_row<T, N>(Y, G, weight, ur, neg_r, e);
            const T t3 = adjoint_row<T, N>(Yd, Gd, weight, ur, neg_r, e);
            const T t4 = adjoint_row<T, N>(Yd, Gd, weight, ur, neg_l, e);
            const T u1 = adjoint_row<T, N>(Y, Gd, weight, ur, neg_l, e);
            const T u2 = adjoint_row<T, N>(Y, Gd, weight, ur, neg_r, e);
            gc = i < s ? ((t1 + t2) + t3) + t4 : gc;
            gdc = i < s ? u1 + u2 : gdc;
            cur ^= 1;
            grow[cur][tid] = gc;
            gdrow[cur][tid] = gdc;
            __syncthreads();
        }
        // Horner: grow[cur] / gdrow[cur] hold w / wd (k = 1: G / Gd themselves), qrow[k & 1] / drow[k & 1] hold q_k / qd_k
        qrow[1][tid] = q[1];
        drow[1][tid] = qd[1];
        __syncthreads();
        T da = T(0);
#pragma unroll
        for (int k = 1; k <= M; ++k) {
            const T* const W = grow[cur] + it0;
            const T* const Wd = gdrow[cur] + it0;
            const T l1 = adjoint_row<T, N>(qrow[k & 1] + it0, W, weight, ur, neg_l, e);
            const T l2 = adjoint_row<T, N>(drow[k & 1] + it0, Wd, weight, ur, neg_l, e);
            da = da + (l1 + l2);
            if (k < M) {
                const T r1 = adjoint_row<T, N>(arow + it0, W, weight, ur, neg_r, e);
                const T r2 = adjoint_row<T, N>(hrow + it0, Wd, weight, ur, neg_r, e);
                const T r3 = adjoint_row<T, N>(arow + it0, Wd, weight, ur, neg_r, e);
                cur ^= 1;
                grow[cur][tid] = (r1 + r2) / T(k + 1);
                gdrow[cur][tid] = r3 / T(k + 1);
                qrow[(k + 1) & 1][tid] = q[k + 1];
                drow[(k + 1) & 1][tid] = qd[k + 1];
                __syncthreads();
            }
        }
        if (live && res_off >= 0) {
            T* d = p.res + item * p.res_stride + res_off;
            *d = (p.beta ? *d : T(0)) + da * scale;
        }
    }
}

}  // namespace gaast
