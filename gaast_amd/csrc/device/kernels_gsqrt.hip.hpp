// kernels_gsqrt.hip.hpp -- the general multivector square root and its reverse mode (GAAST_OP_GSQRT / GAAST_OP_GSQRT_ADJ, gaast_hip.h;
// Step::GSQRT / Step::GSQRT_ADJ; no reference counterpart)
//
//   k_mv_gsqrt<T, N>       res += the principal X with X X = A over a blade set S of N = 2, 4, ... 64 blades (every blade, or the even ones)
//   k_mv_gsqrt_adj<T, N>   res += the cotangent of A, from A and the cotangent g of gsqrt(A)
//   k_mv_gsqrt_jvp<T, N>   res += the tangent of gsqrt at A in direction h (GAAST_OP_GSQRT_JVP; Step::GSQRT_JVP)
//
// The product form of the Denman-Beavers iteration in multivector space, on the left-multiplication matrix L[r][j] = coeff(r, j) A[r xor j]
// of k_mv_inverse (plan.hpp: Step::Inverse, the same blade order and tables).  Per item, as gaast_hip.h states it:
//   M = A, Y = A;  per step:  d = sum_r |(M - e_0)_r| (a butterfly over the item's lanes);  stop when d <= N eps, or one step after
//   d <= sqrt(eps), or a domain error: d not finite, a singular pivot, no stop after K = 16 steps;
//   W = M^-1 (L_M W = e_0);   Y <- 1/2 (Y (e_0 + W));   M <- 1/2 (e_0 + 1/2 (M + W)).
// A step is one multivector inverse and one multivector product, never an N x N matrix product.
//
// Lane layout (both kernels): k_mv_inverse's.  N consecutive lanes own one item, lane r the component of blade S[r] of M and of Y in a
// register each, with copies in LDS; 64 / N items per wave, four waves per workgroup, workgroups stride over the groups of 256 / N items.
//   k_mv_gsqrt      per step lane r gathers row r of L_M from the LDS copy of M into N registers (as k_mv_inverse gathers its row; the
//                   coefficients are kept out of registers the same way) and runs the inverse's elimination on e_0
//                   (GAAST_GSQRT_ELIMINATE below: k_mv_inverse's, statement for statement); the lane that pivoted column c writes W[c] and (e_0 + W)[c]
//                   to LDS; Y (e_0 + W) is gexp's product_row: lane r gathers Y[r xor j] (conflict-free) against the broadcast
//                   (e_0 + W)[j].  The step count differs per item: the loop runs while any item of the workgroup has not stopped
//                   (a ballot per wave, four flags in LDS), an item keeps its Y and M by a select once it has stopped, so the barriers
//                   stay uniform and nothing exits early.
//   k_mv_gsqrt_adj  the forward again, giving X in LDS; then row c of the transposed L_X + R_X in the N registers,
//                   T[c][c xor t] = +-w X[t] +- w X[t] with ADJL's and ADJR's sign bits (w = weight[S[c] & S[t]]; exactly 0 where the two
//                   blades anticommute), the same elimination with right-hand side g_c, and the result on the operand's grades.  A
//                   failed pivot (tested against N eps max |X_i|) or a domain error of the forward (X = NaN) gives NaNs; no count.
//   k_mv_gsqrt_jvp  the adjoint's mirror: the forward again, then row r of L_X + R_X itself in the N registers, built as the forward
//                   builds its row of L_M -- column j holds w X[r xor j], once with L's sign bit and once with the bit of the
//                   right-multiplication matrix R_X[r][j] = coeff(S[j], S[r] xor S[j]) X[r xor j] (same metric factor) -- the same
//                   elimination with right-hand side h_r, and the result on the wanted blades of S.  It takes GsqrtArgs as they are:
//                   cot / cot_stride / g_off are the tangent's rows and offsets, neg_r the sign words of R (neg_l is not read).
// Offsets in int64_t; any row stride (0: one operand shared by every item), padding or alignment takes the same scalar accesses.
#pragma once
#include "kernels_gexp.hip.hpp"

namespace gaast {

template <typename T>
struct GsqrtArgs {
    T* res;
    const T* in;
    const T* cot;             // k_mv_gsqrt_adj: the cotangent rows
    int64_t res_stride, in_stride, cot_stride, batch;
    const int32_t* a_off;     // [N] operand offset of blade j, -1 = absent
    const int32_t* res_off;   // [N] result offset of blade j, -1 = not produced
    const int32_t* g_off;     // [N] cotangent offset of blade j, -1 = absent (k_mv_gsqrt_adj)
    const uint64_t* neg;      // [N] row r: bit j = the reordering sign of L[r][j] is minus
    const uint64_t* neg_l;    // [N] ADJL's sign words (k_mv_gsqrt_adj)
    const uint64_t* neg_r;    // [N] ADJR's sign words (k_mv_gsqrt_adj)
    const T* weight;          // [1 << n] metric factor by shared-vector set
    uint64_t a_neg;           // bit j: operand component j is negated
    int n;                    // dimension of the algebra
    int even;                 // S is the even blades
    int beta;                 // 0: the zero fill of a fresh result is folded in
    unsigned long long* dom;
};

namespace gsqrt_detail {

using namespace gexp_detail;

constexpr int kMaxSteps = 16;

__device__ __forceinline__ float sqrt_eps(float) { return __builtin_sqrtf(1.1920928955078125e-07f); }
__device__ __forceinline__ double sqrt_eps(double) { return 1.4901161193847656e-08; }   // 2^-26

// k_mv_inverse's Gauss-Jordan elimination of [row | RHS] with implicit partial pivoting over the N lanes of an item (lane r holds row r;
// lane0: the item's first lane in the wave), statement for statement as kernels_inverse.hip.hpp describes and has it.  COL: the column
// this lane pivoted, OUT: y of that column, SING: some pivot failed |p| > TOL (the same value in every lane of the item).  No barrier,
// no LDS, no divergence: it runs to the end on whatever values it has.
// A second copy, and a macro: lifted into a __device__ __forceinline__ function (row by reference) the same statements compile to other
// code -- k_mv_inverse<float, 64> then spills 138 SGPRs and k_mv_gsqrt<float, 64> 139, where the text in place spills none (DESIGN.md
// section 16) -- so k_mv_inverse keeps its own text, whose bits and register counts are pinned, and the two kernels here share this one.
#define GAAST_GSQRT_ELIMINATE(row, RHS, TOL, r, lane0, COL, OUT, SING)                                                              \
    {                                                                                                                                \
        constexpr bool WAVE_ = N == 64;                                                                                              \
        T rhs_ = RHS;                                                                                                                \
        const T tol_ = TOL;                                                                                                          \
        bool used_ = false;                                                                                                          \
        uint32_t bad_ = 0;                                                                                                           \
        int my_col_ = r;                                                                                                             \
        T my_piv_ = T(1);                                                                                                            \
        _Pragma("unroll") for (int k_ = 0; k_ < N; ++k_) {                                                                           \
            const T mag_ = abs_m(row[k_]);                                                                                           \
            T best_ = used_ ? T(-1) : (mag_ != mag_ ? T(__builtin_inf()) : mag_);                                                    \
            int who_ = r;                                                                                                            \
            _Pragma("unroll") for (int m_ = N / 2; m_ >= 1; m_ >>= 1) {                                                              \
                const T ob_ = __shfl_xor(best_, m_);                                                                                 \
                const int ow_ = __shfl_xor(who_, m_);                                                                                \
                const bool take_ = (int(ob_ > best_) | (int(ob_ == best_) & int(ow_ < who_))) != 0;                                  \
                best_ = take_ ? ob_ : best_;                                                                                         \
                who_ = take_ ? ow_ : who_;                                                                                           \
            }                                                                                                                        \
            const int src_ = WAVE_ ? __builtin_amdgcn_readfirstlane(who_) : lane0 + who_;                                            \
            const T piv_ = lane_read<WAVE_>(row[k_], src_);                                                                          \
            bad_ |= uint32_t(!(abs_m(piv_) > tol_));                                                                                 \
            asm volatile("" : "+v"(bad_));                                                                                           \
            const bool me_ = who_ == r;                                                                                              \
            if (me_) {                                                                                                               \
                used_ = true;                                                                                                        \
                my_col_ = k_;                                                                                                        \
                my_piv_ = piv_;                                                                                                      \
            }                                                                                                                        \
            const T f_ = me_ ? T(0) : row[k_] / piv_;                                                                                \
            _Pragma("unroll") for (int j_ = k_ + 1; j_ < N; ++j_) {                                                                  \
                row[j_] = fma_m(-f_, lane_read<WAVE_>(row[j_], src_), row[j_]);                                                      \
                if constexpr (WAVE_)                                                                                                 \
                    if ((j_ & 7) == 7) __builtin_amdgcn_sched_barrier(0);                                                            \
            }                                                                                                                        \
            rhs_ = fma_m(-f_, lane_read<WAVE_>(rhs_, src_), rhs_);                                                                   \
        }                                                                                                                            \
        SING = bad_ != 0;                                                                                                            \
        COL = my_col_;                                                                                                               \
        OUT = rhs_ / my_piv_;                                                                                                        \
    }

// the LDS of one workgroup: the copies of M and Y, W and e_0 + W, the metric factors, the per-wave "some item goes on" flags
template <typename T>
struct Shared {
    T m[256], y[256], w[256], z[256];
    T weight[128];
    int go[2][4];
};

// The principal root of the item whose component r is `v` (every lane of the workgroup calls it: the barriers are uniform).  Returns
// the component r of Y; *bad_out: the item is a domain error.  On return a lane may still be reading sh.y / sh.z / sh.w: a barrier comes
// before they are written again.
template <typename T, int N>
__device__ __forceinline__ T principal_root(Shared<T>& sh, T v, bool live, int tid, uint64_t neg, uint32_t e, bool* bad_out) {
    const int r = tid & (N - 1), it0 = tid & ~(N - 1);
    const int lane0 = (tid & 63) & ~(N - 1);
    const T e0 = r == 0 ? T(1) : T(0);
    const T n_eps = T(N) * eps_of(T(0));
    T m = v, y = v;
    // the item's state, bit 0: it has stopped, bit 1: it is a domain error, bit 2: d <= sqrt(eps) at the step before.  An integer made
    // opaque per step, so that it stays in one vector register: as three bools it is three lane masks in SGPRs, live across an
    // elimination that wants every SGPR for the pivot row it broadcasts
    uint32_t st = live ? 0u : 1u;
    __syncthreads();                                    // (every wave has left the loop of the item before: its flags have been read)
#pragma unroll 1
    for (int k = 0;; ++k) {
        T d = abs_m(m - e0);
#pragma unroll
        for (int s = N / 2; s >= 1; s >>= 1) d = d + __shfl_xor(d, s);
        const uint32_t inf = uint32_t(!(d < T(__builtin_inf())));   // d is not finite (a NaN fails the comparison too)
        st |= (inf & ~st & 1u) << 1;                    // not stopped yet and not finite: a domain error
        st |= inf | uint32_t(d <= n_eps) | ((st >> 2) & 1u);
        if (k == kMaxSteps) break;
        const int wave_goes = __builtin_amdgcn_ballot_w64(!(st & 1u)) != 0;   // (by every lane: a ballot sees the active lanes only)
        if ((tid & 63) == 0) sh.go[k & 1][tid >> 6] = wave_goes;
        __syncthreads();                                // (the step before has read sh.y / sh.z; the first: `weight` is written)
        if (!(sh.go[k & 1][0] | sh.go[k & 1][1] | sh.go[k & 1][2] | sh.go[k & 1][3])) break;
        st = (st & 3u) | (uint32_t(d <= sqrt_eps(T(0))) << 2);
        asm volatile("" : "+v"(st));
        sh.m[tid] = m;
        sh.y[tid] = y;
        T amax = abs_m(m);
#pragma unroll
        for (int s = N / 2; s >= 1; s >>= 1) {
            const T o = __shfl_xor(amax, s);
            amax = (int(o > amax) | int(o != o)) ? o : amax;
        }
        __syncthreads();
        // my row of L_M, as k_mv_inverse builds its row (~r and the sign word opaque per pass: the coefficients stay in LDS)
        uint32_t nr = ~uint32_t(r);
        uint32_t neg_lo = uint32_t(neg), neg_hi = uint32_t(neg >> 32);
        asm volatile("" : "+v"(nr), "+v"(neg_lo), "+v"(neg_hi));
        const uint32_t npar = e & ~uint32_t(__builtin_popcount(~nr)) & 1u;   // e & ~parity(r)
        const T* const mine = sh.m + it0;
        T row[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const uint32_t idx = ((uint32_t(j) & nr) << e) | ((uint32_t(__builtin_popcount(uint32_t(j))) & 1u) ? npar : 0u);
            const T c = sh.weight[idx] * mine[(~nr & uint32_t(N - 1)) ^ uint32_t(j)];
            row[j] = flip_sign(c, ((j < 32 ? neg_lo : neg_hi) >> (j & 31)) & 1u);
            if ((j & 7) == 7) __builtin_amdgcn_sched_barrier(0);
        }
        int col;
        bool sing;
        T wc;
        GAAST_GSQRT_ELIMINATE(row, e0, n_eps * amax, r, lane0, col, wc, sing)
        sh.w[it0 + col] = wc;                           // W of the column I pivoted
        sh.z[it0 + col] = (col == 0 ? T(1) : T(0)) + wc;   // e_0 + W
        __syncthreads();
        const T w = sh.w[tid];
        const T yn = T(0.5) * product_row<T, N>(sh.y + it0, sh.z + it0, sh.weight, ~nr, neg, e);
        const T mn = T(0.5) * (e0 + T(0.5) * (m + w));
        st |= (uint32_t(sing) & ~st & 1u) << 1;         // a singular pivot of an item that had not stopped: a domain error
        st |= uint32_t(sing);
        y = (st & 1u) ? y : yn;
        m = (st & 1u) ? m : mn;
    }
    *bad_out = ((st >> 1) | ~st) & 1u;                  // (not stopped after kMaxSteps steps: a domain error too)
    return y;
}

}  // namespace gsqrt_detail

template <typename T, int N>
__global__ __launch_bounds__(256, 2) void k_mv_gsqrt(const GsqrtArgs<T> p) {
    using namespace gsqrt_detail;
    static_assert(N == 2 || N == 4 || N == 8 || N == 16 || N == 32 || N == 64, "one item per N lanes of a wave");
    constexpr int IPB = 256 / N;                 // items of a workgroup
    __shared__ Shared<T> sh;
    const int tid = int(threadIdx.x);
    const int r = tid & (N - 1), g = tid / N;    // my row of the item, my item of the workgroup
    if (tid < (1 << p.n)) sh.weight[tid] = p.weight[tid];
    const int32_t a_off = p.a_off[r], res_off = p.res_off[r];
    const bool a_neg = ((p.a_neg >> r) & 1ULL) != 0;
    const uint64_t neg = p.neg[r];
    const uint32_t e = uint32_t(p.even);
    for (int64_t base = int64_t(blockIdx.x) * IPB; base < p.batch; base += int64_t(gridDim.x) * IPB) {
        const int64_t item = base + g;
        const bool live = item < p.batch;
        T v = T(0);
        if (live && a_off >= 0) v = p.in[item * p.in_stride + a_off];
        if (a_neg) v = -v;
        bool bad;
        const T y = principal_root<T, N>(sh, v, live, tid, neg, e, &bad);
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
__global__ __launch_bounds__(256, 2) void k_mv_gsqrt_adj(const GsqrtArgs<T> p) {
    using namespace gsqrt_detail;
    static_assert(N == 2 || N == 4 || N == 8 || N == 16 || N == 32 || N == 64, "one item per N lanes of a wave");
    constexpr int IPB = 256 / N;
    __shared__ Shared<T> sh;
    const int tid = int(threadIdx.x);
    const int r = tid & (N - 1), g = tid / N, it0 = tid & ~(N - 1);
    const int lane0 = (tid & 63) & ~(N - 1);
    if (tid < (1 << p.n)) sh.weight[tid] = p.weight[tid];
    const int32_t a_off = p.a_off[r], res_off = p.res_off[r], g_off = p.g_off[r];
    const bool a_neg = ((p.a_neg >> r) & 1ULL) != 0;
    const uint64_t neg = p.neg[r], neg_l = p.neg_l[r], neg_r = p.neg_r[r];
    const uint32_t e = uint32_t(p.even);
    const T tol_scale = T(N) * eps_of(T(0));
    for (int64_t base = int64_t(blockIdx.x) * IPB; base < p.batch; base += int64_t(gridDim.x) * IPB) {
        const int64_t item = base + g;
        const bool live = item < p.batch;
        T v = T(0), gv = T(0);
        if (live && a_off >= 0) v = p.in[item * p.in_stride + a_off];
        if (live && g_off >= 0) gv = p.cot[item * p.cot_stride + g_off];
        if (a_neg) v = -v;
        bool bad;
        T x = principal_root<T, N>(sh, v, live, tid, neg, e, &bad);
        x = bad ? qnan(T(0)) : x;                // (a domain error of the forward: every component of the cotangent is NaN by arithmetic)
        __syncthreads();                         // (the last step's product has read sh.y)
        sh.y[tid] = x;
        T amax = abs_m(x);
#pragma unroll
        for (int s = N / 2; s >= 1; s >>= 1) {
            const T o = __shfl_xor(amax, s);
            amax = (int(o > amax) | int(o != o)) ? o : amax;
        }
        __syncthreads();
        // row c = r of the transposed L_X + R_X: T[c][c xor t] = +-w X[t] (ADJL's sign) +- w X[t] (ADJR's), w = weight[S[c] & S[t]]; the
        // factor's index is ((c & t) << e) | (e & parity(c) & parity(t)).  c is opaque per pass, as the row's ~r above
        uint32_t c = uint32_t(r);
        uint32_t l_lo = uint32_t(neg_l), l_hi = uint32_t(neg_l >> 32), r_lo = uint32_t(neg_r), r_hi = uint32_t(neg_r >> 32);
        asm volatile("" : "+v"(c), "+v"(l_lo), "+v"(l_hi), "+v"(r_lo), "+v"(r_hi));
        const uint32_t par = e & uint32_t(__builtin_popcount(c)) & 1u;
        const T* const X = sh.y + it0;
        T row[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const uint32_t t = c ^ uint32_t(j);
            const uint32_t idx = ((c & t) << e) | (uint32_t(__builtin_popcount(t)) & par);
            const T wx = sh.weight[idx] * X[t];
            const uint32_t sl = ((t & 32u) ? l_hi : l_lo) >> (t & 31u), sr = ((t & 32u) ? r_hi : r_lo) >> (t & 31u);
            row[j] = flip_sign(wx, sl & 1u) + flip_sign(wx, sr & 1u);
            if ((j & 7) == 7) __builtin_amdgcn_sched_barrier(0);
        }
        int col;
        bool sing;
        T ac;
        GAAST_GSQRT_ELIMINATE(row, gv, tol_scale * amax, r, lane0, col, ac, sing)
        sh.w[it0 + col] = ac;                    // (sh.w: last read before the forward's final barrier or the one above)
        __syncthreads();
        if (live && res_off >= 0) {
            T* d = p.res + item * p.res_stride + res_off;
            const T a = sing ? qnan(T(0)) : sh.w[tid];
            *d = (p.beta ? *d : T(0)) + a;
        }
    }
}

template <typename T, int N>
__global__ __launch_bounds__(256, 2) void k_mv_gsqrt_jvp(const GsqrtArgs<T> p) {
    using namespace gsqrt_detail;
    static_assert(N == 2 || N == 4 || N == 8 || N == 16 || N == 32 || N == 64, "one item per N lanes of a wave");
    constexpr int IPB = 256 / N;
    __shared__ Shared<T> sh;
    const int tid = int(threadIdx.x);
    const int r = tid & (N - 1), g = tid / N, it0 = tid & ~(N - 1);
    const int lane0 = (tid & 63) & ~(N - 1);
    if (tid < (1 << p.n)) sh.weight[tid] = p.weight[tid];
    const int32_t a_off = p.a_off[r], res_off = p.res_off[r], h_off = p.g_off[r];
    const bool a_neg = ((p.a_neg >> r) & 1ULL) != 0;
    const uint64_t neg = p.neg[r], neg_m = p.neg_r[r];   // row r of L's signs and of R's
    const uint32_t e = uint32_t(p.even);
    const T tol_scale = T(N) * eps_of(T(0));
    for (int64_t base = int64_t(blockIdx.x) * IPB; base < p.batch; base += int64_t(gridDim.x) * IPB) {
        const int64_t item = base + g;
        const bool live = item < p.batch;
        T v = T(0), hv = T(0);
        if (live && a_off >= 0) v = p.in[item * p.in_stride + a_off];
        if (live && h_off >= 0) hv = p.cot[item * p.cot_stride + h_off];
        if (a_neg) v = -v;
        bool bad;
        T x = principal_root<T, N>(sh, v, live, tid, neg, e, &bad);
        x = bad ? qnan(T(0)) : x;                // (a domain error of the forward: every component of the tangent is NaN by arithmetic)
        __syncthreads();                         // (the last step's product has read sh.y)
        sh.y[tid] = x;
        T amax = abs_m(x);
#pragma unroll
        for (int s = N / 2; s >= 1; s >>= 1) {
            const T o = __shfl_xor(amax, s);
            amax = (int(o > amax) | int(o != o)) ? o : amax;
        }
        __syncthreads();
        // my row of L_X + R_X, as principal_root builds its row of L_M: (L + R)[r][j] = +-w X[r xor j] (L's sign) +- w X[r xor j] (R's)
        uint32_t nr = ~uint32_t(r);
        uint32_t l_lo = uint32_t(neg), l_hi = uint32_t(neg >> 32), m_lo = uint32_t(neg_m), m_hi = uint32_t(neg_m >> 32);
        asm volatile("" : "+v"(nr), "+v"(l_lo), "+v"(l_hi), "+v"(m_lo), "+v"(m_hi));
        const uint32_t npar = e & ~uint32_t(__builtin_popcount(~nr)) & 1u;   // e & ~parity(r)
        const T* const X = sh.y + it0;
        T row[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const uint32_t idx = ((uint32_t(j) & nr) << e) | ((uint32_t(__builtin_popcount(uint32_t(j))) & 1u) ? npar : 0u);
            const T wx = sh.weight[idx] * X[(~nr & uint32_t(N - 1)) ^ uint32_t(j)];
            row[j] = flip_sign(wx, ((j < 32 ? l_lo : l_hi) >> (j & 31)) & 1u) + flip_sign(wx, ((j < 32 ? m_lo : m_hi) >> (j & 31)) & 1u);
            if ((j & 7) == 7) __builtin_amdgcn_sched_barrier(0);
        }
        int col;
        bool sing;
        T uc;
        GAAST_GSQRT_ELIMINATE(row, hv, tol_scale * amax, r, lane0, col, uc, sing)
        sh.w[it0 + col] = uc;                    // (sh.w: last read before the forward's final barrier or the one above)
        __syncthreads();
        if (live && res_off >= 0) {
            T* d = p.res + item * p.res_stride + res_off;
            const T u = sing ? qnan(T(0)) : sh.w[tid];
            *d = (p.beta ? *d : T(0)) + u;
        }
    }
}

}  // namespace gaast
