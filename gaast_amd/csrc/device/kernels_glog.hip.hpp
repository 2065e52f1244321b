// kernels_glog.hip.hpp -- the general multivector logarithm and its reverse mode (GAAST_OP_GLOG / GAAST_OP_GLOG_ADJ, gaast_hip.h;
// Step::GLOG / Step::GLOG_ADJ; no reference counterpart)
//
//   k_mv_glog<T, N>       res += the principal logarithm of A over a blade set S of N = 2, 4, ... 64 blades (every blade, or the even ones)
//   k_mv_glog_adj<T, N>   res += the cotangent of A, from A and the cotangent g of glog(A)
//   k_mv_jvp_glog<T, N>   res += the tangent of glog at A in direction h (GAAST_OP_GLOG_JVP; Step::GLOG_JVP)
//   k_mv_adj2_glog<T, N>  res += the gradient in A of <g, that tangent> (GAAST_OP_GLOG_ADJ2; Step::GLOG_ADJ2; at the end of the file)
//
// Inverse scaling and squaring in multivector space, on the left-multiplication matrix of k_mv_inverse (plan.hpp: Step::Inverse, the
// same blade order and tables).  Per item, as gaast_hip.h states it:
//   X_0 = A;  while wmax sum_r |(X_s - e_0)_r| > 1/4 and s < 16:  X_(s+1) = the principal root of X_s (gsqrt_detail::principal_root);
//   E = X_s - e_0;   Y = sum_j alpha_j y_j,  L_(e_0 + beta_j E) y_j = E  (seven eliminations, GAAST_GSQRT_ELIMINATE);   result 2^s Y.
//
// Lane layout (both kernels): k_mv_gsqrt's.  N consecutive lanes own one item, lane r the component of blade S[r]; 64 / N items per
// wave, four waves per workgroup, workgroups stride over the groups of 256 / N items.
//   k_mv_glog      the number of roots differs per item: the root loop runs while any item of the workgroup still roots (a ballot per
//                  wave, four flags in LDS, as principal_root does it for its steps); an item that roots no further passes through the
//                  call with live = false, which returns its argument, and keeps its X by a select.  The barriers stay uniform and
//                  nothing exits early.  One loop (not unrolled) over the seven nodes holds one elimination.
//   k_mv_glog_adj  the forward again, X_1 ... X_s kept in LDS (16 x 256 values); then one loop over the 14 single-transpose solves
//                  (pass 2 j: R_(M_j)^T v = 2^s g with ADJL's sign word, pass 2 j + 1: L_(M_j)^T u = v with ADJR's; a += alpha_j u), and
//                  one loop over the chain i = s ... 1, k_mv_gsqrt_adj's system at X_i.  A failed pivot or a domain error of the
//                  forward gives NaNs; no count.
//   k_mv_jvp_glog  the adjoint read backwards: the forward again with the chain in LDS; one loop up the chain i = 1 ... s,
//                  k_mv_gsqrt_jvp's system (L + R at X_i) on the tangent, an item with fewer roots keeping its value by a select;
//                  then one loop over the 14 solves (pass 2 j: L_(M_j) p = t_s with L's sign word, pass 2 j + 1: R_(M_j) q = p with
//                  the right-multiplication word; acc += alpha_j q), the result scaled by 2^s at the store.  It takes GlogArgs as
//                  they are: cot / cot_stride / g_off are the tangent's rows and offsets, neg_r the sign words of R (neg_l is not read).
//                  (Its name does not begin with k_mv_glog: tests/test_kernel_resources_glog.py counts the kernels whose names do.)
// Offsets in int64_t; any row stride (0: one operand shared by every item), padding or alignment takes the same scalar accesses.
#pragma once
#include "../common/glog_pade.hpp"
#include "kernels_gsqrt.hip.hpp"

namespace gaast {

template <typename T>
struct GlogArgs {
    T* res;
    const T* in;
    const T* cot;             // k_mv_glog_adj: the cotangent rows
    int64_t res_stride, in_stride, cot_stride, batch;
    const int32_t* a_off;     // [N] operand offset of blade j, -1 = absent
    const int32_t* res_off;   // [N] result offset of blade j, -1 = not produced
    const int32_t* g_off;     // [N] cotangent offset of blade j, -1 = absent (k_mv_glog_adj)
    const uint64_t* neg;      // [N] row r: bit j = the reordering sign of L[r][j] is minus
    const uint64_t* neg_l;    // [N] ADJL's sign words (k_mv_glog_adj)
    const uint64_t* neg_r;    // [N] ADJR's sign words (k_mv_glog_adj)
    const T* weight;          // [1 << n] metric factor by shared-vector set
    uint64_t a_neg;           // bit j: operand component j is negated
    T wmax;                   // the largest |weight|
    int n;                    // dimension of the algebra
    int even;                 // S is the even blades
    int beta;                 // 0: the zero fill of a fresh result is folded in
    unsigned long long* dom;
};

namespace glog_detail {

using namespace gsqrt_detail;

// the LDS of a workgroup beside gsqrt_detail::Shared: the quadrature nodes and weights, the per-wave "some item roots on" flags
template <typename T>
struct Extra {
    T node[8], wgt[8];
    int go[2][4];
};

// the adjoint's: the chain X_1 ... X_16 as well
template <typename T>
struct ExtraAdj {
    T chain[kGlogMaxRoots][256];
    T node[8], wgt[8];
    int go[2][4];
};

template <typename T, typename X>
__device__ __forceinline__ void load_pade(X& ex, int tid) {
#pragma unroll
    for (int j = 0; j < kGlogPadeTerms; ++j)
        if (tid == j) {
            ex.node[j] = T(kGlogPadeNode[j]);
            ex.wgt[j] = T(kGlogPadeWeight[j]);
        }
}

// max_i |v_i| over the item's lanes (a NaN wins), as principal_root takes it
template <typename T, int N>
__device__ __forceinline__ T item_amax(T v) {
    T amax = abs_m(v);
#pragma unroll
    for (int s = N / 2; s >= 1; s >>= 1) {
        const T o = __shfl_xor(amax, s);
        amax = (int(o > amax) | int(o != o)) ? o : amax;
    }
    return amax;
}

// The roots of the item whose component r is `v`: on return *x_out is the component r of X_s, *s_out is s, *bad_out a domain error
// so far (a non-finite component, a root's domain error, still beyond 1/4 after 16 roots).  CHAIN: X_(i+1) of every item is stored
// to chain[i][tid] for i < the returned count (the largest s of the workgroup; an item with fewer roots repeats its X_s).
// Every lane of the workgroup calls it: the barriers are uniform.
template <typename T, int N, bool CHAIN, typename X>
__device__ __forceinline__ int take_roots(Shared<T>& sh, X& ex, T v, bool live, int tid, uint64_t neg, uint32_t e, T wmax, T* x_out, int* s_out,
                                          bool* bad_out) {
    const int r = tid & (N - 1);
    const T e0 = r == 0 ? T(1) : T(0);
    T x = v;
    int s = 0, it = 0;
    uint32_t bad = 0;
#pragma unroll 1
    for (;; ++it) {
        T d = abs_m(x - e0);
#pragma unroll
        for (int m = N / 2; m >= 1; m >>= 1) d = d + __shfl_xor(d, m);
        d = d * wmax;
        bad |= uint32_t(!(d < T(__builtin_inf())));          // not finite (a NaN fails the comparison too)
        const bool need = live && !bad && d > T(kGlogTheta);
        if (it == kGlogMaxRoots) {
            bad |= uint32_t(need);                           // s would exceed 16
            break;
        }
        const int wave_goes = __builtin_amdgcn_ballot_w64(need) != 0;
        if ((tid & 63) == 0) ex.go[it & 1][tid >> 6] = wave_goes;
        __syncthreads();
        if (!(ex.go[it & 1][0] | ex.go[it & 1][1] | ex.go[it & 1][2] | ex.go[it & 1][3])) break;
        uint32_t nd = uint32_t(need);                        // (in a vector register across the root: a lane mask would sit in SGPRs its elimination wants)
        asm volatile("" : "+v"(nd));
        bool rbad;
        const T xr = principal_root<T, N>(sh, x, nd != 0, tid, neg, e, &rbad);
        asm volatile("" : "+v"(nd));
        x = nd ? xr : x;
        bad |= nd & uint32_t(rbad);
        s += int(nd);
        if constexpr (CHAIN) ex.chain[it][tid] = x;
        asm volatile("" : "+v"(bad), "+v"(s));
    }
    *x_out = x;
    *s_out = s;
    *bad_out = bad != 0;
    return it;
}

}  // namespace glog_detail

template <typename T, int N>
__global__ __launch_bounds__(256, 2) void k_mv_glog(const GlogArgs<T> p) {
    using namespace glog_detail;
    static_assert(N == 2 || N == 4 || N == 8 || N == 16 || N == 32 || N == 64, "one item per N lanes of a wave");
    constexpr int IPB = 256 / N;                 // items of a workgroup
    __shared__ Shared<T> sh;
    __shared__ Extra<T> ex;
    const int tid = int(threadIdx.x);
    const int r = tid & (N - 1), g = tid / N, it0 = tid & ~(N - 1);
    const int lane0 = (tid & 63) & ~(N - 1);
    if (tid < (1 << p.n)) sh.weight[tid] = p.weight[tid];
    load_pade<T>(ex, tid);
    const int32_t a_off = p.a_off[r], res_off = p.res_off[r];
    const bool a_neg = ((p.a_neg >> r) & 1ULL) != 0;
    const uint64_t neg = p.neg[r];
    const uint32_t e = uint32_t(p.even);
    const T e0 = r == 0 ? T(1) : T(0);
    const T n_eps = T(N) * eps_of(T(0));
    for (int64_t base = int64_t(blockIdx.x) * IPB; base < p.batch; base += int64_t(gridDim.x) * IPB) {
        const int64_t item = base + g;
        const bool live = item < p.batch;
        T v = T(0);
        if (live && a_off >= 0) v = p.in[item * p.in_stride + a_off];
        if (a_neg) v = -v;
        T x;
        int s;
        bool bad;
        take_roots<T, N, false>(sh, ex, v, live, tid, neg, e, p.wmax, &x, &s, &bad);
        const T E = x - e0;
        T acc = T(0);
        uint32_t pbad = 0;
#pragma unroll 1
        for (int j = 0; j < kGlogPadeTerms; ++j) {           // acc += alpha_j y_j,  L_(e_0 + beta_j E) y_j = E
            __syncthreads();                                 // (the pass before has read sh.m; the first: the roots are over, `node` is written)
            const T mj = e0 + ex.node[j] * E;
            sh.m[tid] = mj;
            const T amax = item_amax<T, N>(mj);
            __syncthreads();
            // my row of L_(M_j), as principal_root builds its row
            uint32_t nr = ~uint32_t(r);
            uint32_t neg_lo = uint32_t(neg), neg_hi = uint32_t(neg >> 32);
            asm volatile("" : "+v"(nr), "+v"(neg_lo), "+v"(neg_hi));
            const uint32_t npar = e & ~uint32_t(__builtin_popcount(~nr)) & 1u;   // e & ~parity(r)
            const T* const mine = sh.m + it0;
            T row[N];
#pragma unroll
            for (int c = 0; c < N; ++c) {
                const uint32_t idx = ((uint32_t(c) & nr) << e) | ((uint32_t(__builtin_popcount(uint32_t(c))) & 1u) ? npar : 0u);
                const T w = sh.weight[idx] * mine[(~nr & uint32_t(N - 1)) ^ uint32_t(c)];
                row[c] = flip_sign(w, ((c < 32 ? neg_lo : neg_hi) >> (c & 31)) & 1u);
                if ((c & 7) == 7) __builtin_amdgcn_sched_barrier(0);
            }
            int col;
            bool sing;
            T yc;
            GAAST_GSQRT_ELIMINATE(row, E, n_eps * amax, r, lane0, col, yc, sing)
            sh.w[it0 + col] = yc;
            __syncthreads();
            acc = fma_m(ex.wgt[j], sh.w[tid], acc);
            pbad |= uint32_t(sing);
            asm volatile("" : "+v"(pbad));
        }
        bad = bad || pbad != 0;
        if (live) {
            if (res_off >= 0) {
                T* d = p.res + item * p.res_stride + res_off;
                *d = bad ? qnan(T(0)) : (p.beta ? *d : T(0)) + ldexp_m(acc, s);
            }
            if (bad && r == 0) atomicAdd(p.dom, 1ull);
        }
    }
}

template <typename T, int N>
__global__ __launch_bounds__(256, 2) void k_mv_glog_adj(const GlogArgs<T> p) {
    using namespace glog_detail;
    static_assert(N == 2 || N == 4 || N == 8 || N == 16 || N == 32 || N == 64, "one item per N lanes of a wave");
    constexpr int IPB = 256 / N;
    __shared__ Shared<T> sh;
    __shared__ ExtraAdj<T> ex;
    const int tid = int(threadIdx.x);
    const int r = tid & (N - 1), g = tid / N, it0 = tid & ~(N - 1);
    const int lane0 = (tid & 63) & ~(N - 1);
    if (tid < (1 << p.n)) sh.weight[tid] = p.weight[tid];
    load_pade<T>(ex, tid);
    const int32_t a_off = p.a_off[r], res_off = p.res_off[r], g_off = p.g_off[r];
    const bool a_neg = ((p.a_neg >> r) & 1ULL) != 0;
    const uint64_t neg = p.neg[r], neg_l = p.neg_l[r], neg_r = p.neg_r[r];
    const uint32_t e = uint32_t(p.even);
    const T e0 = r == 0 ? T(1) : T(0);
    const T n_eps = T(N) * eps_of(T(0));
    for (int64_t base = int64_t(blockIdx.x) * IPB; base < p.batch; base += int64_t(gridDim.x) * IPB) {
        const int64_t item = base + g;
        const bool live = item < p.batch;
        T v = T(0), gv = T(0);
        if (live && a_off >= 0) v = p.in[item * p.in_stride + a_off];
        if (live && g_off >= 0) gv = p.cot[item * p.cot_stride + g_off];
        if (a_neg) v = -v;
        T x;
        int s;
        bool bad;
        const int smax = take_roots<T, N, true>(sh, ex, v, live, tid, neg, e, p.wmax, &x, &s, &bad);
        const T E = x - e0;
        const T gs = ldexp_m(gv, s);                         // g' = 2^s g
        T a = T(0), rhs = gs;
        uint32_t pbad = uint32_t(bad);
#pragma unroll 1
        for (int ps = 0; ps < 2 * kGlogPadeTerms; ++ps) {    // pass 2 j: R_(M_j)^T v = g';  pass 2 j + 1: L_(M_j)^T u = v,  a += alpha_j u
            const int j = ps >> 1;
            const bool second = (ps & 1) != 0;
            __syncthreads();                                 // (the pass before has read sh.m; the first: the roots are over, `node` is written)
            const T mj = e0 + ex.node[j] * E;
            sh.m[tid] = mj;
            const T amax = item_amax<T, N>(mj);
            __syncthreads();
            // row c = r of the single transpose: T[c][c xor t] = +-w M[t], w = weight[S[c] & S[t]], with ADJL's sign bit for R_M^T and
            // ADJR's for L_M^T (the two halves of k_mv_gsqrt_adj's row)
            uint32_t c = uint32_t(r);
            uint32_t s_lo = second ? uint32_t(neg_r) : uint32_t(neg_l), s_hi = second ? uint32_t(neg_r >> 32) : uint32_t(neg_l >> 32);
            asm volatile("" : "+v"(c), "+v"(s_lo), "+v"(s_hi));
            const uint32_t par = e & uint32_t(__builtin_popcount(c)) & 1u;
            const T* const M = sh.m + it0;
            T row[N];
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const uint32_t t = c ^ uint32_t(k);
                const uint32_t idx = ((c & t) << e) | (uint32_t(__builtin_popcount(t)) & par);
                const T wx = sh.weight[idx] * M[t];
                row[k] = flip_sign(wx, (((t & 32u) ? s_hi : s_lo) >> (t & 31u)) & 1u);
                if ((k & 7) == 7) __builtin_amdgcn_sched_barrier(0);
            }
            int col;
            bool sing;
            T oc;
            GAAST_GSQRT_ELIMINATE(row, rhs, n_eps * amax, r, lane0, col, oc, sing)
            sh.w[it0 + col] = oc;
            __syncthreads();
            const T sol = sh.w[tid];
            a = second ? fma_m(ex.wgt[j], sol, a) : a;
            rhs = second ? gs : sol;
            pbad |= uint32_t(sing);
            asm volatile("" : "+v"(pbad));
        }
#pragma unroll 1
        for (int i = smax; i >= 1; --i) {                    // a <- the solution of ADJL(a, X_i) + ADJR(a, X_i) = a, for i <= s
            const T* const X = ex.chain[i - 1] + it0;
            const T amax = item_amax<T, N>(ex.chain[i - 1][tid]);
            uint32_t c = uint32_t(r);
            uint32_t l_lo = uint32_t(neg_l), l_hi = uint32_t(neg_l >> 32), r_lo = uint32_t(neg_r), r_hi = uint32_t(neg_r >> 32);
            asm volatile("" : "+v"(c), "+v"(l_lo), "+v"(l_hi), "+v"(r_lo), "+v"(r_hi));
            const uint32_t par = e & uint32_t(__builtin_popcount(c)) & 1u;
            T row[N];
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const uint32_t t = c ^ uint32_t(k);
                const uint32_t idx = ((c & t) << e) | (uint32_t(__builtin_popcount(t)) & par);
                const T wx = sh.weight[idx] * X[t];
                const uint32_t sl = ((t & 32u) ? l_hi : l_lo) >> (t & 31u), sr = ((t & 32u) ? r_hi : r_lo) >> (t & 31u);
                row[k] = flip_sign(wx, sl & 1u) + flip_sign(wx, sr & 1u);
                if ((k & 7) == 7) __builtin_amdgcn_sched_barrier(0);
            }
            int col;
            bool sing;
            T oc;
            GAAST_GSQRT_ELIMINATE(row, a, n_eps * amax, r, lane0, col, oc, sing)
            __syncthreads();                                 // (sh.w: the pass before has been read)
            sh.w[it0 + col] = oc;
            __syncthreads();
            const bool mine = i <= s;
            a = mine ? sh.w[tid] : a;
            pbad |= uint32_t(mine && sing);
            asm volatile("" : "+v"(pbad));
        }
        if (live && res_off >= 0) {
            T* d = p.res + item * p.res_stride + res_off;
            *d = (p.beta ? *d : T(0)) + (pbad ? qnan(T(0)) : a);
        }
    }
}

template <typename T, int N>
__global__ __launch_bounds__(256, 2) void k_mv_jvp_glog(const GlogArgs<T> p) {
    using namespace glog_detail;
    static_assert(N == 2 || N == 4 || N == 8 || N == 16 || N == 32 || N == 64, "one item per N lanes of a wave");
    constexpr int IPB = 256 / N;
    __shared__ Shared<T> sh;
    __shared__ ExtraAdj<T> ex;
    const int tid = int(threadIdx.x);
    const int r = tid & (N - 1), g = tid / N, it0 = tid & ~(N - 1);
    const int lane0 = (tid & 63) & ~(N - 1);
    if (tid < (1 << p.n)) sh.weight[tid] = p.weight[tid];
    load_pade<T>(ex, tid);
    const int32_t a_off = p.a_off[r], res_off = p.res_off[r], h_off = p.g_off[r];
    const bool a_neg = ((p.a_neg >> r) & 1ULL) != 0;
    const uint64_t neg = p.neg[r], neg_m = p.neg_r[r];   // row r of L's signs and of R's
    const uint32_t e = uint32_t(p.even);
    const T e0 = r == 0 ? T(1) : T(0);
    const T n_eps = T(N) * eps_of(T(0));
    for (int64_t base = int64_t(blockIdx.x) * IPB; base < p.batch; base += int64_t(gridDim.x) * IPB) {
        const int64_t item = base + g;
        const bool live = item < p.batch;
        T v = T(0), hv = T(0);
        if (live && a_off >= 0) v = p.in[item * p.in_stride + a_off];
        if (live && h_off >= 0) hv = p.cot[item * p.cot_stride + h_off];
        if (a_neg) v = -v;
        T x;
        int s;
        bool bad;
        const int smax = take_roots<T, N, true>(sh, ex, v, live, tid, neg, e, p.wmax, &x, &s, &bad);
        const T E = x - e0;
        T t = hv;
        uint32_t pbad = uint32_t(bad);
        __syncthreads();                                     // (the chain is written: after 16 roots no barrier follows the last store)
#pragma unroll 1
        for (int i = 1; i <= smax; ++i) {                    // t <- the solution of (L + R at X_i) t = t, for i <= s
            const T* const X = ex.chain[i - 1] + it0;
            const T amax = item_amax<T, N>(ex.chain[i - 1][tid]);
            uint32_t nr = ~uint32_t(r);
            uint32_t l_lo = uint32_t(neg), l_hi = uint32_t(neg >> 32), m_lo = uint32_t(neg_m), m_hi = uint32_t(neg_m >> 32);
            asm volatile("" : "+v"(nr), "+v"(l_lo), "+v"(l_hi), "+v"(m_lo), "+v"(m_hi));
            const uint32_t npar = e & ~uint32_t(__builtin_popcount(~nr)) & 1u;   // e & ~parity(r)
            T row[N];
#pragma unroll
            for (int c = 0; c < N; ++c) {
                const uint32_t idx = ((uint32_t(c) & nr) << e) | ((uint32_t(__builtin_popcount(uint32_t(c))) & 1u) ? npar : 0u);
                const T wx = sh.weight[idx] * X[(~nr & uint32_t(N - 1)) ^ uint32_t(c)];
                row[c] = flip_sign(wx, ((c < 32 ? l_lo : l_hi) >> (c & 31)) & 1u) + flip_sign(wx, ((c < 32 ? m_lo : m_hi) >> (c & 31)) & 1u);
                if ((c & 7) == 7) __builtin_amdgcn_sched_barrier(0);
            }
            int col;
            bool sing;
            T oc;
            GAAST_GSQRT_ELIMINATE(row, t, n_eps * amax, r, lane0, col, oc, sing)
            __syncthreads();                                 // (sh.w: the pass before has been read)
            sh.w[it0 + col] = oc;
            __syncthreads();
            const bool mine = i <= s;
            t = mine ? sh.w[tid] : t;
            pbad |= uint32_t(mine && sing);
            asm volatile("" : "+v"(pbad));
        }
        T acc = T(0), rhs = t;
#pragma unroll 1
        for (int ps = 0; ps < 2 * kGlogPadeTerms; ++ps) {    // pass 2 j: L_(M_j) p = t_s;  pass 2 j + 1: R_(M_j) q = p,  acc += alpha_j q
            const int j = ps >> 1;
            const bool second = (ps & 1) != 0;
            __syncthreads();                                 // (the pass before has read sh.m and sh.w; the first: the chain is over, `node` is written)
            const T mj = e0 + ex.node[j] * E;
            sh.m[tid] = mj;
            const T amax = item_amax<T, N>(mj);
            __syncthreads();
            // my row of L_(M_j) or of R_(M_j), as principal_root builds its row: +-w M[r xor c] with L's sign word or R's
            uint32_t nr = ~uint32_t(r);
            uint32_t s_lo = second ? uint32_t(neg_m) : uint32_t(neg), s_hi = second ? uint32_t(neg_m >> 32) : uint32_t(neg >> 32);
            asm volatile("" : "+v"(nr), "+v"(s_lo), "+v"(s_hi));
            const uint32_t npar = e & ~uint32_t(__builtin_popcount(~nr)) & 1u;   // e & ~parity(r)
            const T* const M = sh.m + it0;
            T row[N];
#pragma unroll
            for (int c = 0; c < N; ++c) {
                const uint32_t idx = ((uint32_t(c) & nr) << e) | ((uint32_t(__builtin_popcount(uint32_t(c))) & 1u) ? npar : 0u);
                const T w = sh.weight[idx] * M[(~nr & uint32_t(N - 1)) ^ uint32_t(c)];
                row[c] = flip_sign(w, ((c < 32 ? s_lo : s_hi) >> (c & 31)) & 1u);
                if ((c & 7) == 7) __builtin_amdgcn_sched_barrier(0);
            }
            int col;
            bool sing;
            T oc;
            GAAST_GSQRT_ELIMINATE(row, rhs, n_eps * amax, r, lane0, col, oc, sing)
            sh.w[it0 + col] = oc;
            __syncthreads();
            const T sol = sh.w[tid];
            acc = second ? fma_m(ex.wgt[j], sol, acc) : acc;
            rhs = second ? t : sol;
            pbad |= uint32_t(sing);
            asm volatile("" : "+v"(pbad));
        }
        if (live && res_off >= 0) {
            T* d = p.res + item * p.res_stride + res_off;
            *d = (p.beta ? *d : T(0)) + (pbad ? qnan(T(0)) : ldexp_m(acc, s));
        }
    }
}

// ---- second order: GAAST_OP_GLOG_ADJ2 ----------------------------------------------------------------------------------------------
// GlogArgs plus the second row pointer, its stride and offsets, and the fourth sign table: the three kernels above keep their argument bytes
template <typename T>
struct GlogAdj2Args {
    T* res;
    const T* in;
    const T* cot;             // the rows of g
    const T* tan;             // the rows of h
    int64_t res_stride, in_stride, cot_stride, tan_stride, batch;
    const int32_t* a_off;     // [N] operand offset of blade j, -1 = absent
    const int32_t* res_off;   // [N] result offset of blade j, -1 = not produced
    const int32_t* g_off;     // [N] offset of blade j in the rows of g, -1 = absent
    const int32_t* h_off;     // [N] offset of blade j in the rows of h, -1 = absent
    const uint64_t* neg;      // [N] the sign words of L
    const uint64_t* neg_l;    // [N] ADJL's sign words (the rows of R^T)
    const uint64_t* neg_r;    // [N] ADJR's sign words (the rows of L^T)
    const uint64_t* neg_m;    // [N] the sign words of R
    const T* weight;          // [1 << n] metric factor by shared-vector set
    uint64_t a_neg;           // bit j: operand component j is negated
    T wmax;                   // the largest |weight|
    int n;                    // dimension of the algebra
    int even;                 // S is the even blades
    int beta;                 // 0: the zero fill of a fresh result is folded in
};

namespace glog_detail {

// the LDS of k_mv_adj2_glog beside Shared and ExtraAdj: the tangents t_1 ... t_16, and three values of each lane that no elimination needs
// in a register (g' = 2^s g, t_s, gamma)
template <typename T>
struct ExtraAdj2 {
    T tchain[kGlogMaxRoots][256];
    T park[3][256];
};

// Component c of ADJR(G1, Q) + ADJL(G2, Q) of one item (Q, G1, G2: its N values in LDS): the single-transpose row of Q that
// k_mv_glog_adj builds, T[c][c xor t] = +-w Q[t], with ADJR's sign word (row c of L_Q^T) against G1 and with ADJL's (row c of R_Q^T)
// against G2.  2 N multiply-adds, no elimination.
template <typename T, int N>
__device__ __forceinline__ T adjoint_pair(const T* Q, const T* G1, const T* G2, const T* weight, uint32_t c, uint32_t e, uint64_t neg_l, uint64_t neg_r) {
    uint32_t l_lo = uint32_t(neg_l), l_hi = uint32_t(neg_l >> 32), r_lo = uint32_t(neg_r), r_hi = uint32_t(neg_r >> 32);
    asm volatile("" : "+v"(c), "+v"(l_lo), "+v"(l_hi), "+v"(r_lo), "+v"(r_hi));
    const uint32_t par = e & uint32_t(__builtin_popcount(c)) & 1u;
    T acc = T(0);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const uint32_t t = c ^ uint32_t(k);
        const uint32_t idx = ((c & t) << e) | (uint32_t(__builtin_popcount(t)) & par);
        const T wq = weight[idx] * Q[t];
        const uint32_t sl = ((t & 32u) ? l_hi : l_lo) >> (t & 31u), sr = ((t & 32u) ? r_hi : r_lo) >> (t & 31u);
        acc = fma_m(flip_sign(wq, sr & 1u), G1[k], acc);
        acc = fma_m(flip_sign(wq, sl & 1u), G2[k], acc);
    }
    return acc;
}

}  // namespace glog_detail

// k_mv_adj2_glog<T, N>  res += the gradient in A of <g, GLOG_JVP(h, A)> (GAAST_OP_GLOG_ADJ2, gaast_hip.h; Step::GLOG_ADJ2), k_mv_glog_adj's
// lane layout.  The forward again with the chain X_1 ... X_s in LDS; k_mv_jvp_glog's loop up the chain, every t_i kept in a second chain;
// one loop over the 35 Pade solves, five per node -- pass 0: R_M^T v1 = g', 1: L_M^T u = v1, 2: L_M^T v2 = g', 3: L_M p = t_s,
// 4: R_M q = p -- the row form (single transpose or plain) and the sign word chosen per pass, a += alpha u after pass 1 and
// gamma -= alpha beta (ADJR(v1, q) + ADJL(v2, q)) after pass 4 (adjoint_pair on v1, v2 and q in LDS); then one loop down the chain with two
// solves of k_mv_gsqrt_adj's system per level, w <- S_i^-T w and e <- S_i^-T (e - (ADJR(w, t_i) + ADJL(w, t_i))).  An item with fewer
// roots keeps its values by a select; the barriers stay uniform and nothing exits early.  A failed pivot or a domain error of the
// forward gives NaNs; no count.
// (Its name does not contain k_mv_glog: tests/test_kernel_resources_glog.py counts the kernels whose names do.)
template <typename T, int N>
__global__ __launch_bounds__(256, 2) void k_mv_adj2_glog(const GlogAdj2Args<T> p) {
    using namespace glog_detail;
    static_assert(N == 2 || N == 4 || N == 8 || N == 16 || N == 32 || N == 64, "one item per N lanes of a wave");
    constexpr int IPB = 256 / N;
    __shared__ Shared<T> sh;
    __shared__ ExtraAdj<T> ex;
    __shared__ ExtraAdj2<T> ex2;
    const int tid = int(threadIdx.x);
    const int r = tid & (N - 1), g = tid / N, it0 = tid & ~(N - 1);
    const int lane0 = (tid & 63) & ~(N - 1);
    if (tid < (1 << p.n)) sh.weight[tid] = p.weight[tid];
    load_pade<T>(ex, tid);
    const int32_t a_off = p.a_off[r], res_off = p.res_off[r], g_off = p.g_off[r], h_off = p.h_off[r];
    const bool a_neg = ((p.a_neg >> r) & 1ULL) != 0;
    const uint64_t neg = p.neg[r], neg_l = p.neg_l[r], neg_r = p.neg_r[r], neg_m = p.neg_m[r];   // row r of L's signs, of ADJL's, of ADJR's and of R's
    const uint32_t e = uint32_t(p.even);
    const T e0 = r == 0 ? T(1) : T(0);
    const T n_eps = T(N) * eps_of(T(0));
    for (int64_t base = int64_t(blockIdx.x) * IPB; base < p.batch; base += int64_t(gridDim.x) * IPB) {
        const int64_t item = base + g;
        const bool live = item < p.batch;
        T v = T(0), gv = T(0), hv = T(0);
        if (live && a_off >= 0) v = p.in[item * p.in_stride + a_off];
        if (live && g_off >= 0) gv = p.cot[item * p.cot_stride + g_off];
        if (live && h_off >= 0) hv = p.tan[item * p.tan_stride + h_off];
        if (a_neg) v = -v;
        T x;
        int s;
        bool bad;
        const int smax = take_roots<T, N, true>(sh, ex, v, live, tid, neg, e, p.wmax, &x, &s, &bad);
        const T E = x - e0;
        uint32_t pbad = uint32_t(bad);
        ex2.park[0][tid] = ldexp_m(gv, s);                   // g' = 2^s g
        __syncthreads();                                     // (the chain is written: after 16 roots no barrier follows the last store)
        {
            T t = hv;
#pragma unroll 1
            for (int i = 1; i <= smax; ++i) {                // t <- the solution of (L + R at X_i) t = t, for i <= s; t_i kept
                const T* const X = ex.chain[i - 1] + it0;
                const T amax = item_amax<T, N>(ex.chain[i - 1][tid]);
                uint32_t nr = ~uint32_t(r);
                uint32_t l_lo = uint32_t(neg), l_hi = uint32_t(neg >> 32), m_lo = uint32_t(neg_m), m_hi = uint32_t(neg_m >> 32);
                asm volatile("" : "+v"(nr), "+v"(l_lo), "+v"(l_hi), "+v"(m_lo), "+v"(m_hi));
                const uint32_t npar = e & ~uint32_t(__builtin_popcount(~nr)) & 1u;   // e & ~parity(r)
                T row[N];
#pragma unroll
                for (int c = 0; c < N; ++c) {
                    const uint32_t idx = ((uint32_t(c) & nr) << e) | ((uint32_t(__builtin_popcount(uint32_t(c))) & 1u) ? npar : 0u);
                    const T wx = sh.weight[idx] * X[(~nr & uint32_t(N - 1)) ^ uint32_t(c)];
                    row[c] = flip_sign(wx, ((c < 32 ? l_lo : l_hi) >> (c & 31)) & 1u) + flip_sign(wx, ((c < 32 ? m_lo : m_hi) >> (c & 31)) & 1u);
                    if ((c & 7) == 7) __builtin_amdgcn_sched_barrier(0);
                }
                int col;
                bool sing;
                T oc;
                GAAST_GSQRT_ELIMINATE(row, t, n_eps * amax, r, lane0, col, oc, sing)
                __syncthreads();                             // (sh.w: the pass before has been read)
                sh.w[it0 + col] = oc;
                __syncthreads();
                const bool mine = i <= s;
                t = mine ? sh.w[tid] : t;
                ex2.tchain[i - 1][tid] = t;
                pbad |= uint32_t(mine && sing);
                asm volatile("" : "+v"(pbad));
            }
            ex2.park[1][tid] = t;                            // t_s
        }
        ex2.park[2][tid] = T(0);                             // gamma
        T a = T(0), rhs = ex2.park[0][tid];
#pragma unroll 1
        for (int ps = 0; ps < 5 * kGlogPadeTerms; ++ps) {    // node j, pass k (above)
            const int j = (ps * 13) >> 6, k = ps - 5 * j;    // ps / 5 and ps % 5 for ps < 35
            __syncthreads();                                 // (the pass before has read sh.m, sh.w, sh.y, sh.z; the first: the chain is over, `node` is written)
            const T mj = e0 + ex.node[j] * E;
            sh.m[tid] = mj;
            const T amax = item_amax<T, N>(mj);
            __syncthreads();
            // Column c of my row is +-w M[r xor c] in both forms.  Single transpose (passes 0 ... 2), T[r][r xor t] = +-w M[t]: w = weight[S[r] & S[t]],
            // the sign bit t = r xor c of ADJL's word (R_M^T) or ADJR's (L_M^T).  Plain (passes 3, 4), as principal_root builds its row:
            // w = weight[S[c] & ~S[r]], the sign bit c of L's word or R's.  One text: x = c xor (r or 0), w = weight[S[x] & S[r or ~r]], bit x.
            const bool tr = k < 3;
            const uint64_t word = k == 0 ? neg_l : k == 3 ? neg : k == 4 ? neg_m : neg_r;
            uint32_t rr = uint32_t(r);
            asm volatile("" : "+v"(rr));
            uint32_t xr = tr ? rr : 0u, ym = tr ? rr : ~rr;
            uint32_t s_lo = uint32_t(word), s_hi = uint32_t(word >> 32);
            asm volatile("" : "+v"(xr), "+v"(ym), "+v"(s_lo), "+v"(s_hi));
            const uint32_t pp = e & (tr ? uint32_t(__builtin_popcount(rr)) : ~uint32_t(__builtin_popcount(rr))) & 1u;
            const T* const M = sh.m + it0;
            T row[N];
#pragma unroll
            for (int c = 0; c < N; ++c) {
                const uint32_t xx = xr ^ uint32_t(c);
                const uint32_t idx = ((xx & ym) << e) | (uint32_t(__builtin_popcount(xx)) & pp);
                const T wm = sh.weight[idx] * M[(rr & uint32_t(N - 1)) ^ uint32_t(c)];
                row[c] = flip_sign(wm, (((xx & 32u) ? s_hi : s_lo) >> (xx & 31u)) & 1u);
                if ((c & 7) == 7) __builtin_amdgcn_sched_barrier(0);
            }
            int col;
            bool sing;
            T oc;
            GAAST_GSQRT_ELIMINATE(row, rhs, n_eps * amax, r, lane0, col, oc, sing)
            sh.w[it0 + col] = oc;
            __syncthreads();
            const T sol = sh.w[tid];
            pbad |= uint32_t(sing);
            asm volatile("" : "+v"(pbad));
            int kq = k;                                      // (opaque: seeing the k of the word's choice again, the compiler specialises the
            asm volatile("" : "+s"(kq));                     //  whole pass per value of k, and <T, 64> then spills some 230 SGPRs.  What a
                                                             //  compiler makes of this may change: tests/test_kernel_resources_glog_adj2.py
                                                             //  fails on any spill of any instantiation)
            if (kq == 0) {                                   // v1
                sh.y[tid] = sol;
                rhs = sol;
            } else if (kq == 1) {                            // u
                a = fma_m(ex.wgt[j], sol, a);
                rhs = ex2.park[0][tid];
            } else if (kq == 2) {                            // v2
                sh.z[tid] = sol;
                rhs = ex2.park[1][tid];
            } else if (kq == 3) {                            // p
                rhs = sol;
            } else {                                         // q, in sh.w
                const T pair = adjoint_pair<T, N>(sh.w + it0, sh.y + it0, sh.z + it0, sh.weight, uint32_t(r), e, neg_l, neg_r);
                ex2.park[2][tid] = fma_m(-(ex.wgt[j] * ex.node[j]), pair, ex2.park[2][tid]);
                rhs = ex2.park[0][tid];
            }
        }
        T w = a, ev = ex2.park[2][tid];
#pragma unroll 1
        for (int i2 = 2 * smax + 1; i2 >= 2; --i2) {         // level i = i2 / 2 = s ... 1: first w (i2 odd), then e with the new w (i2 even)
            const int i = i2 >> 1;
            const bool second = (i2 & 1) == 0;
            const T* const X = ex.chain[i - 1] + it0;
            const T amax = item_amax<T, N>(ex.chain[i - 1][tid]);
            uint32_t c = uint32_t(r);
            T rhs2 = w;
            if (second) rhs2 = ev - adjoint_pair<T, N>(ex2.tchain[i - 1] + it0, sh.w + it0, sh.w + it0, sh.weight, c, e, neg_l, neg_r);   // (sh.w: the new w)
            uint32_t l_lo = uint32_t(neg_l), l_hi = uint32_t(neg_l >> 32), r_lo = uint32_t(neg_r), r_hi = uint32_t(neg_r >> 32);
            asm volatile("" : "+v"(c), "+v"(l_lo), "+v"(l_hi), "+v"(r_lo), "+v"(r_hi));
            const uint32_t par = e & uint32_t(__builtin_popcount(c)) & 1u;
            T row[N];
#pragma unroll
            for (int kk = 0; kk < N; ++kk) {
                const uint32_t t = c ^ uint32_t(kk);
                const uint32_t idx = ((c & t) << e) | (uint32_t(__builtin_popcount(t)) & par);
                const T wx = sh.weight[idx] * X[t];
                const uint32_t sl = ((t & 32u) ? l_hi : l_lo) >> (t & 31u), sr = ((t & 32u) ? r_hi : r_lo) >> (t & 31u);
                row[kk] = flip_sign(wx, sl & 1u) + flip_sign(wx, sr & 1u);
                if ((kk & 7) == 7) __builtin_amdgcn_sched_barrier(0);
            }
            int col;
            bool sing;
            T oc;
            GAAST_GSQRT_ELIMINATE(row, rhs2, n_eps * amax, r, lane0, col, oc, sing)
            __syncthreads();                                 // (sh.w: the pass before has been read)
            sh.w[it0 + col] = oc;
            __syncthreads();
            const bool mine = i <= s;
            const T sol = sh.w[tid];
            w = (mine && !second) ? sol : w;
            ev = (mine && second) ? sol : ev;
            pbad |= uint32_t(mine && sing);
            asm volatile("" : "+v"(pbad));
        }
        if (live && res_off >= 0) {
            T* d = p.res + item * p.res_stride + res_off;
            *d = (p.beta ? *d : T(0)) + (pbad ? qnan(T(0)) : ev);
        }
    }
}

}  // namespace gaast
