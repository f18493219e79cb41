// colsum.h — the two fixed-order column-sum kernels shared by backward.hip (mumpy_col_sum_fwd) and gemm_bwd.hip (the bias
// gradient of a Linear backward that wants no dW).  Each including translation unit gets its own copy.
#pragma once
#include "common.h"

namespace {

// out[c] (+)= sum_p partial[p * stride + c]: 64 columns per block, 16 lane groups each summing every 16th partial, combined
// through LDS in group order -- a fixed summation tree (bitwise reproducible) without a thousands-long serial chain
__global__ __launch_bounds__(1024) void partial_reduce_kernel(const float* __restrict__ partial, float* __restrict__ out,
                                                              int64_t nparts, int64_t width, int64_t stride, int accum) {
    __shared__ float red[16][64];
    const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * 64 + col;
    float s = 0.f;
    if (i < width && grp < nparts)
        s = mumpy::ordered_sum(partial[grp * stride + i], partial + (grp + 16) * stride + i, 16 * stride, (int)((nparts - grp + 15) / 16) - 1);
    red[grp][col] = s;
    __syncthreads();
    if (grp == 0 && i < width) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) t += red[g][col];
        out[i] = accum ? out[i] + t : t;
    }
}

// column sums of a (R, C) matrix: stage 1 writes one partial row per block of rows.  A block is 64 columns x 4 row lanes
// (coalesced 256-B row segments, 4 rows in flight per column); the 4 row lanes are combined in order through LDS.
__global__ __launch_bounds__(256) void col_sum_partial_kernel(const float* __restrict__ x, float* __restrict__ partial, int64_t R,
                                                              int C, int rows_per_block) {
    __shared__ float red[4][64];
    const int col = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
    const int c = blockIdx.x * 64 + col;
    float s = 0.f;
    if (c < C)
        for (int64_t r = r0 + rl; r < r0 + rows_per_block && r < R; r += 4) s += x[r * C + c];
    red[rl][col] = s;
    __syncthreads();
    if (rl == 0 && c < C) partial[(int64_t)blockIdx.y * C + c] = (red[0][col] + red[1][col]) + (red[2][col] + red[3][col]);
}

}  // namespace
