// kernels_linmap.hip.hpp -- outermorphisms of a linear map of the vector space, applied to a batch of graded rows
//
//   out(item)_k = M_k . in(item)_k   for every grade k of the row, M_k = C_k(M) (the k-th compound, common/metric_basis.hpp)
//
// shared by every item.  This is the change of basis of programs in a non-diagonal metric (gaast_hip_program_create_in_basis) and
// the public gaast_hip_linmap_apply.  The matrices of all grades sit in one device array, grade k at moff[k], row-major
// C(n,k) x C(n,k).  Grade 0 is the 1 x 1 matrix (1) and grade n the 1 x 1 matrix (det M): the same code is a copy and a scale there.
// Two regimes:
//   k_linmap_small   n <= 6 (C(n,k) <= 20): memory-bound.  All matrices in LDS (<= 924 entries), 64 items per workgroup staged through
//                    LDS with coalesced (16-byte when the rows are contiguous and aligned) row loads and stores; a wave computes one
//                    component of 64 items, so its matrix reads are broadcasts.  Persistent grid.
//   k_linmap_mfma    n >= 7: per grade a GEMM  out_k[items x R] = in_k[items x K] . M_k^T  on v_mfma_{f32,f64}_16x16x4, 64 items x
//                    64 output components per workgroup (2 x 2 waves, 2 x 2 tiles of 16 x 16 each), K in steps of 32 through LDS.
//                    blockIdx.x walks the (grade, output-column tile) jobs fastest, so the workgroups that read one slab of
//                    input rows run together and the rows come from L2; blockIdx.y walks item tiles.
// Sums are fused multiply-add chains in increasing input-component order (the f32 MFMA is bit-for-bit such a chain).
//
// Reverse mode with respect to the matrix (gaast_hip_linmap_matrix_vjp, n <= 8), two launches:
//   k_linmap_outer_sum       W_k[I][J] = sum_items g_k[item][I] x_k[item][J] per grade k >= 1, reduced over one chunk of items
//   k_linmap_minor_contract  dL/dM[i][j] = sum of sign * C_{k-1}(M)[I \ i][J \ j] * W_k[I][J] over a host-built term table
// with k_sum_rows (kernels_reduce.hip.hpp) between them when the batch spans more than one chunk.
#pragma once
#include "kernels_common.hip.hpp"

namespace gaast {

constexpr int kLinmapMaxGrades = 17;
constexpr int kLinmapSmallComps = 64;   // row length limit of k_linmap_small (n <= 6)
constexpr int kLinmapItems = 64;        // items per workgroup of k_linmap_small
constexpr int kLinmapBM = 64, kLinmapBN = 64, kLinmapKT = 32;

template <typename T>
struct LinmapArgs {
    const T* in;
    T* out;
    const T* mats;
    int64_t in_stride, out_stride, batch;
    int row_len, n_grades, mat_total, n_jobs;
    int in_vec, out_vec;                       // small: 16-byte row I/O (contiguous, aligned rows)
    int goff[kLinmapMaxGrades];                // per present grade: offset in the row, C(n,k), offset of its matrix
    int glen[kLinmapMaxGrades];
    int moff[kLinmapMaxGrades];
    int job0[kLinmapMaxGrades + 1];            // mfma: first output-column tile of each present grade (prefix sums)
    uint32_t comp[kLinmapSmallComps];          // small: per row component: grade offset | local row << 7 | C(n,k) << 13 | moff << 19
};

template <typename T>
__global__ __launch_bounds__(256) void k_linmap_small(LinmapArgs<T> p) {
    extern __shared__ __align__(16) unsigned char linmap_lds[];
    T* mats = reinterpret_cast<T*>(linmap_lds);
    const int mpad = (p.mat_total + 3) & ~3;
    const int ls = p.row_len + 1;              // padded item stride in LDS: the 64 lanes of a wave read 64 items' component c
    T* tin = mats + mpad;
    T* tout = tin + kLinmapItems * ls;
    __shared__ uint32_t comp[kLinmapSmallComps];
    const int tid = threadIdx.x;
    for (int i = tid; i < p.mat_total; i += 256) mats[i] = p.mats[i];
    if (tid < p.row_len) comp[tid] = p.comp[tid];
    constexpr int V = 16 / sizeof(T);
    typedef T vec_t __attribute__((ext_vector_type(V)));
    const int item = tid & (kLinmapItems - 1), cg = tid >> 6;
    for (int64_t t0 = int64_t(blockIdx.x) * kLinmapItems; t0 < p.batch; t0 += int64_t(gridDim.x) * kLinmapItems) {
        const int cnt = int(p.batch - t0 < kLinmapItems ? p.batch - t0 : kLinmapItems);
        const int total = cnt * p.row_len;
        if (p.in_vec) {
            const vec_t* src = reinterpret_cast<const vec_t*>(p.in + t0 * p.in_stride);
            for (int v = tid; v * V < total; v += 256) {
                const int e = v * V, it = e / p.row_len, c = e - it * p.row_len;
                const vec_t x = src[v];
#pragma unroll
                for (int j = 0; j < V; ++j) tin[it * ls + c + j] = x[j];
            }
        } else {
            for (int e = tid; e < total; e += 256) {
                const int it = e / p.row_len, c = e - it * p.row_len;
                tin[it * ls + c] = p.in[(t0 + it) * p.in_stride + c];
            }
        }
        __syncthreads();
        if (item < cnt) {
            const T* x = tin + item * ls;
            for (int c = cg; c < p.row_len; c += 4) {
                const uint32_t w = comp[c];
                const int goff = int(w & 127u), r = int((w >> 7) & 63u), len = int((w >> 13) & 63u), mo = int(w >> 19);
                const T* m = mats + mo + r * len;
                T acc = T(0);
                for (int j = 0; j < len; ++j) acc = fma(m[j], x[goff + j], acc);
                tout[item * ls + c] = acc;
            }
        }
        __syncthreads();
        if (p.out_vec) {
            vec_t* dst = reinterpret_cast<vec_t*>(p.out + t0 * p.out_stride);
            for (int v = tid; v * V < total; v += 256) {
                const int e = v * V, it = e / p.row_len, c = e - it * p.row_len;
                vec_t y;
#pragma unroll
                for (int j = 0; j < V; ++j) y[j] = tout[it * ls + c + j];
                dst[v] = y;
            }
        } else {
            for (int e = tid; e < total; e += 256) {
                const int it = e / p.row_len, c = e - it * p.row_len;
                p.out[(t0 + it) * p.out_stride + c] = tout[it * ls + c];
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_linmap_mfma(LinmapArgs<T> p) {
    typedef Mfma16x4<T> F;
    constexpr int KP = kLinmapKT + 1;          // padded LDS rows: the 16 lanes of a fragment read 16 different rows
    __shared__ T sa[kLinmapBM * KP];           // input rows: [item][k]
    __shared__ T sb[kLinmapBN * KP];           // matrix rows: [output component][k]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int job = blockIdx.x;
    int g = 0;
    while (g + 1 < p.n_grades && p.job0[g + 1] <= job) ++g;
    const int goff = p.goff[g], K = p.glen[g], R = K;
    const T* M = p.mats + p.moff[g];
    const int r0 = (job - p.job0[g]) * kLinmapBN;
    const int lr = tid >> 2, lk = (tid & 3) * 8;   // loader: one row, eight consecutive k
    const int fi = lane & 15, fk = lane >> 4;      // fragment: row / column fi, k = 4 s + fk
    for (int64_t i0 = int64_t(blockIdx.y) * kLinmapBM; i0 < p.batch; i0 += int64_t(gridDim.y) * kLinmapBM) {
        typename F::acc_t acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) acc[a][b] = typename F::acc_t{0, 0, 0, 0};
        const bool item_ok = i0 + lr < p.batch;
        const T* arow = p.in + (i0 + lr) * p.in_stride + goff;
        const bool r_ok = r0 + lr < R;
        const T* brow = M + int64_t(r0 + lr) * K;
        for (int k0 = 0; k0 < K; k0 += kLinmapKT) {
            T va[8], vb[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = k0 + lk + j;
                va[j] = (item_ok && k < K) ? arow[k] : T(0);
                vb[j] = (r_ok && k < K) ? brow[k] : T(0);
            }
            __syncthreads();   // the previous step's fragments have been read
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                sa[lr * KP + lk + j] = va[j];
                sb[lr * KP + lk + j] = vb[j];
            }
            __syncthreads();
#pragma unroll
            for (int s = 0; s < kLinmapKT / 4; ++s) {
                const int k = 4 * s + fk;
                T fa[2], fb[2];
#pragma unroll
                for (int a = 0; a < 2; ++a) fa[a] = sa[(wm * 32 + a * 16 + fi) * KP + k];
#pragma unroll
                for (int b = 0; b < 2; ++b) fb[b] = sb[(wn * 32 + b * 16 + fi) * KP + k];
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) acc[a][b] = F::mma(fa[a], fb[b], acc[a][b]);
            }
        }
        // accumulator register v of lane (fi, fk): item row F::row(fk, v) of the tile, output column fi
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int r = r0 + wn * 32 + b * 16 + fi;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int64_t it = i0 + wm * 32 + a * 16 + F::row(fk, v);
                    if (it < p.batch && r < R) p.out[it * p.out_stride + goff + r] = acc[a][b][v];
                }
            }
    }
}

// ---- reverse mode with respect to the matrix ------------------------------------------------------------------------------------
constexpr int kOuterChunk = 1024;        // items per partial (= GAAST_SUM_ROWS_CHUNK: the first level of the fixed tree)
constexpr int kOuterWaves = 4;           // 16 x 16 tiles of W per workgroup, one per wave
constexpr int kContractThreads = 256;    // interleaved chains per entry of dL/dM
constexpr int kContractIndexBits = 14;   // a term word: index into W | index into the compounds << 14 | negative << 28

template <typename T>
struct OuterSumArgs {
    const T* g;                                // cotangent rows
    const T* x;                                // input rows
    T* out;                                    // [chunk][w_total]: W of every present grade >= 1, grade g at woff[g], row-major
    int64_t g_stride, x_stride, batch;
    int w_total, n_tiles, n_grades;
    int goff[kLinmapMaxGrades];                // per present grade >= 1: offset in the row, C(n,k), offset of its W
    int glen[kLinmapMaxGrades];
    int woff[kLinmapMaxGrades];
    int tile0[kLinmapMaxGrades + 1];           // first tile of each present grade (prefix sums of ceil(C(n,k) / 16)^2)
};

// One wave per 16 x 16 tile of W_k and chunk of kOuterChunk items, K = items, on v_mfma_{f32,f64}_16x16x4: lane (fi, fk) of a step
// reads g[item0 + fk][I0 + fi] and x[item0 + fk][J0 + fi] straight from the rows (item-major rows ARE the K-major operands: the 16
// lanes of a group read 16 consecutive elements of one row), element by element, so any stride and element alignment is the same
// code.  One accumulator per tile, the steps issued in item order: the sum of an entry is ONE chain over the chunk's items in item
// order, four per instruction (the instruction adds its four products onto the accumulator in k = item order, as k_linmap_mfma's
// note on the f32 MFMA states), whatever the grid -- the fixed first level of the tree.  Rows and columns beyond C(n,k) and items
// beyond the chunk enter as exact zeros (selected, never multiplied in from memory) and are not stored.
template <typename T>
__global__ __launch_bounds__(64 * kOuterWaves) void k_linmap_outer_sum(OuterSumArgs<T> p) {
    typedef Mfma16x4<T> F;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = int(blockIdx.x) * kOuterWaves + wave;
    if (tile >= p.n_tiles) return;             // (uniform over the wave; the kernel has no barrier)
    int gi = 0;
    while (gi + 1 < p.n_grades && p.tile0[gi + 1] <= tile) ++gi;
    const int len = p.glen[gi], tl = (len + 15) >> 4, t = tile - p.tile0[gi];
    const int I0 = (t / tl) * 16, J0 = (t % tl) * 16;
    const int fi = lane & 15, fk = lane >> 4;
    const bool i_ok = I0 + fi < len, j_ok = J0 + fi < len;
    const int64_t b0 = int64_t(blockIdx.y) * kOuterChunk;
    const int64_t b1 = b0 + kOuterChunk < p.batch ? b0 + kOuterChunk : p.batch;
    const int64_t gcol = p.goff[gi] + I0 + fi, xcol = p.goff[gi] + J0 + fi;
    typename F::acc_t acc = typename F::acc_t{0, 0, 0, 0};
    for (int64_t b = b0; b < b1; b += 16) {
        T a[4], c[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int64_t item = b + 4 * s + fk;
            const bool ok = item < b1;
            a[s] = (ok && i_ok) ? p.g[item * p.g_stride + gcol] : T(0);
            c[s] = (ok && j_ok) ? p.x[item * p.x_stride + xcol] : T(0);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = F::mma(a[s], c[s], acc);
    }
    // accumulator register v of lane (fi, fk): row I0 + F::row(fk, v) of the tile, column J0 + fi
    T* w = p.out + int64_t(blockIdx.y) * p.w_total + p.woff[gi];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int I = I0 + F::row(fk, v);
        if (I < len && j_ok) w[I * len + J0 + fi] = acc[v];
    }
}

// One workgroup per entry (i, j) of dL/dM.  Its terms terms[row_start[ij] .. row_start[ij + 1]) are ordered by grade, I, J; lane t
// adds terms t, t + 256, ... in that order (product rounded, then added: no contraction), then the 256 partial sums are joined by
// the fixed binary tree part[t] += part[t + 128], + 64, ... + 1.
template <typename T>
__global__ __launch_bounds__(kContractThreads) void k_linmap_minor_contract(const T* __restrict__ w, const T* __restrict__ mats,
                                                                            const uint32_t* __restrict__ terms,
                                                                            const uint32_t* __restrict__ row_start, T* __restrict__ dm) {
    __shared__ T part[kContractThreads];
    const int tid = threadIdx.x;
    const uint32_t e0 = row_start[blockIdx.x], e1 = row_start[blockIdx.x + 1];
    constexpr uint32_t kMask = (1u << kContractIndexBits) - 1u;
    T acc = T(0);
    for (uint32_t e = e0 + uint32_t(tid); e < e1; e += kContractThreads) {
        const uint32_t t = terms[e];
        const T term = mats[(t >> kContractIndexBits) & kMask] * w[t & kMask];
        acc += (t >> (2 * kContractIndexBits)) ? -term : term;
    }
    part[tid] = acc;
    __syncthreads();
    for (int off = kContractThreads / 2; off > 0; off >>= 1) {
        if (tid < off) part[tid] += part[tid + off];
        __syncthreads();
    }
    if (tid == 0) dm[blockIdx.x] = part[0];
}

}  // namespace gaast
