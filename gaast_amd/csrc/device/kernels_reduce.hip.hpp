// kernels_reduce.hip.hpp -- deterministic sum of the rows of a batch (gaast_hip_mv_sum_rows): the gradient of an input shared by
// every item is the sum of its per-item gradients.
//
// A fixed two-level tree.  Level 1: workgroup (x = chunk, y = column tile) sums the rows [x * chunk, (x + 1) * chunk) of its columns
// in row order into one partial row; level 2 is the same kernel over the partial rows with one chunk holding all of them.  Every
// sum is the same sequential chain whatever the grid, CU count or timing, so the bits depend on the batch and the data only.
// Rows pass through LDS kSumTile elements at a time: the workgroup loads them coalesced (16-byte vectors when the tile is one
// contiguous, aligned span), then lane c adds column c of the staged rows into its register in row order.  No atomics.
#pragma once
#include "kernels_common.hip.hpp"

namespace gaast {

constexpr int kSumTile = 4096;   // elements staged per step (32 KiB in f64)
constexpr int kSumCols = 256;    // columns per workgroup = lanes that add

template <typename T>
__global__ __launch_bounds__(256) void k_sum_rows(const T* __restrict__ in, int64_t stride, int64_t rows, int row_len, int64_t chunk,
                                                  T* __restrict__ out, int64_t out_stride) {
    __shared__ __align__(16) T tile[kSumTile];
    const int tc = row_len < kSumCols ? row_len : kSumCols;   // tile width
    const int j0 = int(blockIdx.y) * tc;
    const int ncol = row_len - j0 < tc ? row_len - j0 : tc;
    const int R = kSumTile / tc;                               // rows per step
    const int64_t r0 = int64_t(blockIdx.x) * chunk;
    const int64_t r1 = r0 + chunk < rows ? r0 + chunk : rows;
    const int tid = threadIdx.x;
    constexpr int V = 16 / sizeof(T);
    typedef T vec_t __attribute__((ext_vector_type(V)));
    T acc = T(0);
    for (int64_t rb = r0; rb < r1; rb += R) {
        const int nr = int(r1 - rb < R ? r1 - rb : R);
        if (ncol == row_len && stride == row_len) {
            // whole rows, back to back: one span of nr * row_len elements
            const T* src = in + rb * row_len;
            const int cnt = nr * row_len;
            int done = 0;
            if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
                const vec_t* vs = reinterpret_cast<const vec_t*>(src);
                vec_t* vt = reinterpret_cast<vec_t*>(tile);
                for (int v = tid; v < cnt / V; v += 256) vt[v] = __builtin_nontemporal_load(vs + v);
                done = cnt / V * V;
            }
            for (int e = done + tid; e < cnt; e += 256) tile[e] = src[e];
        } else {
            for (int e = tid; e < nr * ncol; e += 256) {
                const int r = e / ncol, c = e - r * ncol;
                tile[r * tc + c] = in[(rb + r) * stride + j0 + c];
            }
        }
        __syncthreads();
        if (tid < ncol)
            for (int r = 0; r < nr; ++r) acc += tile[r * tc + tid];
        __syncthreads();
    }
    if (tid < ncol) out[int64_t(blockIdx.x) * out_stride + j0 + tid] = acc;
}

}  // namespace gaast
