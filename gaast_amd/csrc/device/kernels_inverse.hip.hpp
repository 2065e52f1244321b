// kernels_inverse.hip.hpp -- the general multivector inverse (GAAST_OP_INV, gaast_hip.h; Step::INVERSE; no reference counterpart)
//
//   k_mv_inverse<T, N>   res += the Y with A Y = 1 over a blade set S of N = 2, 4, ... 64 blades (every blade, or the even ones)
//
// Y solves L y = e_0 with the left-multiplication matrix L[r][j] = coeff(r, j) A[r xor j] (plan.hpp: Step::Inverse; S in ascending
// bitmask order, S[j] = j or (j << 1) | parity(j), so that the index of S[r] xor S[j] is r xor j in both sets).
//
// Lane layout: N consecutive lanes own one item, lane r holding row r of [L | e_0] in registers -- N values of T and the right-hand
// side; 64 / N items per wave, four waves per workgroup, workgroups stride over the groups of 256 / N items.  The column index of
// every loop is a compile-time constant: the loops unroll fully and no register is indexed at run time (N = 64 in f64: 128 VGPRs for
// the row).  An item's operand row goes through LDS: lane r loads the component of blade S[r] (absent grades read as 0; the lanes of
// a wave cover the contiguous rows of its items, so the loads coalesce into those rows' cache lines), then gathers its N entries
// A[r xor j] with their signs (the reordering sign from a 64-bit word per row, the metric factor from a table by shared-vector set).
// Gauss-Jordan elimination with IMPLICIT partial pivoting: rows never move, a lane remembers that it has been a pivot and for
// which column.  The pivot of column k is the largest |L[r][k]| over the lanes not used yet, found by a butterfly over the N lanes
// (ties: the lowest lane, so the result does not depend on the order of the reduction; a NaN counts as the largest and is taken at
// once); the pivot row's remaining entries are broadcast to the item's lanes -- v_readlane with the pivot lane in an SGPR at
// N = 64, where it is wave-uniform, ds_bpermute below that -- and every other row, used or not, eliminates column k.  At the end
// the lane that pivoted column k holds y_k = rhs / pivot; the y go back through LDS so that lane r stores the component of blade
// S[r], again into contiguous rows.
// An item is singular when at any column !(|pivot| > N eps max_i |A_i|) (NaN pivots included): every produced component of it is a
// quiet NaN and it is counted once in *dom (gaast_hip_program_domain_errors).  Its elimination still runs to the end on whatever
// values it has: ordinary arithmetic, no early exit, no divergence between the items of a wave.
// Offsets in int64_t; any row stride (0: one operand shared by every item), padding or alignment takes the same code.
#pragma once
#include "kernels_common.hip.hpp"

namespace gaast {

template <typename T>
struct InverseArgs {
    T* res;
    const T* in;
    int64_t res_stride, in_stride, batch;
    const int32_t* a_off;     // [N] operand offset of blade j, -1 = absent
    const int32_t* res_off;   // [N] result offset of blade j, -1 = not produced
    const uint64_t* neg;      // [N] row r: bit j = the reordering sign of L[r][j] is minus
    const T* weight;          // [1 << n] metric factor by shared-vector set
    uint64_t a_neg;           // bit j: operand component j is negated
    int n;                    // dimension of the algebra
    int even;                 // S is the even blades
    int beta;                 // 0: the zero fill of a fresh result is folded in
    unsigned long long* dom;
};

namespace inverse_detail {

__device__ __forceinline__ float eps_of(float) { return 1.1920928955078125e-07f; }
__device__ __forceinline__ double eps_of(double) { return 2.220446049250313e-16; }
__device__ __forceinline__ float abs_m(float x) { return __builtin_fabsf(x); }
__device__ __forceinline__ double abs_m(double x) { return __builtin_fabs(x); }
__device__ __forceinline__ float fma_m(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_m(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float qnan(float) { return __builtin_nanf(""); }
__device__ __forceinline__ double qnan(double) { return __builtin_nan(""); }

// x with its sign flipped when bit 0 of `flip` is set: integer arithmetic on the sign bit (a select would keep a lane mask per column)
__device__ __forceinline__ float flip_sign(float x, uint32_t flip) { return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, x) ^ (flip << 31)); }
__device__ __forceinline__ double flip_sign(double x, uint32_t flip) { return __builtin_bit_cast(double, __builtin_bit_cast(uint64_t, x) ^ (uint64_t(flip) << 63)); }

// the value lane `src` holds (an absolute lane of the wave).  WAVE: src is wave-uniform and sits in an SGPR.
template <bool WAVE>
__device__ __forceinline__ int lane_read(int v, int src) {
    if constexpr (WAVE) return __builtin_amdgcn_readlane(v, src);
    else return __builtin_amdgcn_ds_bpermute(src << 2, v);
}
template <bool WAVE>
__device__ __forceinline__ float lane_read(float v, int src) {
    return __builtin_bit_cast(float, lane_read<WAVE>(__builtin_bit_cast(int, v), src));
}
template <bool WAVE>
__device__ __forceinline__ double lane_read(double v, int src) {
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = uint32_t(lane_read<WAVE>(int(uint32_t(u)), src)), hi = uint32_t(lane_read<WAVE>(int(uint32_t(u >> 32)), src));
    return __builtin_bit_cast(double, uint64_t(lo) | (uint64_t(hi) << 32));
}

}  // namespace inverse_detail

template <typename T, int N>
__global__ __launch_bounds__(256) void k_mv_inverse(const InverseArgs<T> p) {
    using namespace inverse_detail;
    static_assert(N == 2 || N == 4 || N == 8 || N == 16 || N == 32 || N == 64, "one item per N lanes of a wave");
    constexpr int IPB = 256 / N;                 // items of a workgroup
    constexpr bool WAVE = N == 64;
    __shared__ T rows[256];                      // [IPB][N]: an item's operand by blade index, later its inverse
    __shared__ T weight[128];
    const int tid = int(threadIdx.x);
    const int r = tid & (N - 1), g = tid / N;    // my row of the item, my item of the workgroup
    const int lane0 = (tid & 63) & ~(N - 1);     // first lane of my item in the wave
    if (tid < (1 << p.n)) weight[tid] = p.weight[tid];
    const int32_t a_off = p.a_off[r], res_off = p.res_off[r];
    const bool a_neg = ((p.a_neg >> r) & 1ULL) != 0;
    const uint64_t neg = p.neg[r];
    T* const mine = rows + g * N;
    const T tol_scale = T(N) * eps_of(T(0));
    for (int64_t base = int64_t(blockIdx.x) * IPB; base < p.batch; base += int64_t(gridDim.x) * IPB) {
        const int64_t item = base + g;
        const bool live = item < p.batch;
        T v = T(0);
        if (live && a_off >= 0) v = p.in[item * p.in_stride + a_off];
        if (a_neg) v = -v;
        __syncthreads();                         // (the previous group's inverse has been read; the first pass: `weight` is written)
        mine[r] = v;
        T amax = abs_m(v);
#pragma unroll
        for (int m = N / 2; m >= 1; m >>= 1) {
            const T o = __shfl_xor(amax, m);
            amax = (int(o > amax) | int(o != o)) ? o : amax;   // (a NaN component makes the threshold NaN: the item is singular)
        }
        __syncthreads();
        // my row of [L | e_0].  The metric factor's index is S[j] & ~S[r] = ((j & ~r) << e) | (e & parity(j) & ~parity(r)), e = p.even.
        // Nothing here depends on the item, so the compiler would compute the N coefficients once and keep them in N more
        // registers than the row itself: ~r is made opaque per pass (an empty asm statement, no instruction), which keeps the
        // coefficients where they are cheap to rebuild -- LDS
        uint32_t nr = ~uint32_t(r);
        uint32_t neg_lo = uint32_t(neg), neg_hi = uint32_t(neg >> 32);
        asm volatile("" : "+v"(nr), "+v"(neg_lo), "+v"(neg_hi));
        const uint32_t e = uint32_t(p.even), npar = e & ~uint32_t(__builtin_popcount(~nr)) & 1u;   // e & ~parity(r)
        T row[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const uint32_t idx = ((uint32_t(j) & nr) << e) | ((uint32_t(__builtin_popcount(uint32_t(j))) & 1u) ? npar : 0u);
            const T c = weight[idx] * mine[(~nr & uint32_t(N - 1)) ^ uint32_t(j)];
            row[j] = flip_sign(c, ((j < 32 ? neg_lo : neg_hi) >> (j & 31)) & 1u);
            if ((j & 7) == 7) __builtin_amdgcn_sched_barrier(0);   // (else all 2 N loads of the gather are in flight at once, each in a register)
        }
        T rhs = r == 0 ? T(1) : T(0);
        __syncthreads();                         // (every lane has gathered: `mine` takes the inverse from here on)
        const T tol = tol_scale * amax;
        bool used = false;
        uint32_t bad = 0;                        // some pivot failed the test
        int my_col = r;
        T my_piv = T(1);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            // the pivot lane: the largest |row[k]| among the lanes not used yet, the lowest lane among equals; a NaN is the largest
            const T mag = abs_m(row[k]);
            T best = used ? T(-1) : (mag != mag ? T(__builtin_inf()) : mag);
            int who = r;
#pragma unroll
            for (int m = N / 2; m >= 1; m >>= 1) {
                const T ob = __shfl_xor(best, m);
                const int ow = __shfl_xor(who, m);
                const bool take = (int(ob > best) | (int(ob == best) & int(ow < who))) != 0;   // (no short circuit: one basic block per item)
                best = take ? ob : best;
                who = take ? ow : who;
            }
            const int src = WAVE ? __builtin_amdgcn_readfirstlane(who) : lane0 + who;
            const T piv = lane_read<WAVE>(row[k], src);
            bad |= uint32_t(!(abs_m(piv) > tol));
            asm volatile("" : "+v"(bad));      // (tested now: left alone, the compiler keeps all N pivots until the end)
            const bool me = who == r;
            if (me) {
                used = true;
                my_col = k;
                my_piv = piv;
            }
            const T f = me ? T(0) : row[k] / piv;
#pragma unroll
            for (int j = k + 1; j < N; ++j) {
                row[j] = fma_m(-f, lane_read<WAVE>(row[j], src), row[j]);
                // (v_readlane results live in SGPRs: keep the scheduler from reading a whole pivot row ahead of its use)
                if constexpr (WAVE)
                    if ((j & 7) == 7) __builtin_amdgcn_sched_barrier(0);
            }
            rhs = fma_m(-f, lane_read<WAVE>(rhs, src), rhs);
        }
        const bool singular = bad != 0;
        mine[my_col] = rhs / my_piv;             // y of the column I pivoted (my_col < N whatever the values were)
        __syncthreads();
        if (live) {
            if (res_off >= 0) {
                T* d = p.res + item * p.res_stride + res_off;
                const T y = singular ? qnan(T(0)) : mine[r];
                *d = singular ? y : (p.beta ? *d : T(0)) + y;
            }
            if (singular && r == 0) atomicAdd(p.dom, 1ull);
        }
    }
}

}  // namespace gaast
