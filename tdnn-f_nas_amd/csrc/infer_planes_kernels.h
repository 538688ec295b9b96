// infer_planes_kernels.h -- the small kernels around the plane GEMMs of the f16x3 inference (host side: infer_planes.hip, the f16x3 reader of infer_forward.hip's schedule).  The GEMM itself
// is planes_gemm_kernel<.., POST = true> (planes_gemm_kernels.h); the splits are those of planes_split.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

namespace tdnnf {
namespace {

constexpr int kInferBoundBlocks = 64;  // partial sums of a norm bound (what planes_scale_bound sums)

// block sum of `acc` over 256 threads into out[blockIdx.x] (fixed order)
__device__ __forceinline__ void infer_block_sum(double acc, double *out) {
  __shared__ double red[4];
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// out[b] = block b's share of the n per-row-tile, per-column sums of squares a plane GEMM left (PlanesGemmArgs::colstats): together
// the squared Frobenius norm of the matrix it stored
__global__ __launch_bounds__(256) void infer_stats_bound_kernel(const float *sumsq, long long n, double *out) {
  double acc = 0;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < n; e += gridDim.x * 256LL) acc += (double)sumsq[e];
  infer_block_sum(acc, out);
}

// the same partial sums from a pass over the matrix (an activation no plane GEMM stored, split into more than one plane buffer)
__global__ __launch_bounds__(256) void infer_sumsq_kernel(MatView x, double *out) {
  const long long total = (long long)x.rows * x.cols;
  double acc = 0;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const float v = x.data[(e / x.cols) * x.stride + e % x.cols];
    acc += (double)v * v;
  }
  infer_block_sum(acc, out);
}

// out[n][t * Dp + k] = W[n][t * Di + k] for k < Di, 0 for Di <= k < Dp: every tap's column block of a weight matrix at its own
// 16-aligned K block (Dp = Di rounded up to 16; out is Do x K Dp, dense)
__global__ __launch_bounds__(256) void infer_pad_taps_kernel(const float *W, int ldw, int Do, int K, int Di, int Dp, float *out) {
  const long long total = (long long)Do * K * Dp;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int n = (int)(e / (K * Dp)), c = (int)(e % (K * Dp)), t = c / Dp, k = c % Dp;
    out[e] = k < Di ? W[(long long)n * ldw + t * Di + k] : 0.f;
  }
}

}  // namespace
}  // namespace tdnnf
