// den_dev.h -- device helpers that several of the denominator's kernel families share (den_persistent_kernels.h, den_mw_kernels.h,
// den_wide_kernels.h): the workgroup sum, the clamped exponential, a frame's output row one frame ahead, the sum over a sliced-ELL row.
#pragma once
#include "chain_types.h"

namespace tdnnf {
namespace {

constexpr int kDenThreads = 1024;
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float block_sum(float v, float *red, int nwaves) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();  // protect red from the previous use
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
  for (int w = 0; w < nwaves; w++) s += red[w];
  return s;
}

// ApplyExpLimited(-30, 30): comparisons (not fmin/fmax) so that a NaN stays a NaN and trips the
// objf-not-finite failure path, as in the reference stack.
__device__ __forceinline__ float exp_limited(float v) {
  v = v < -30.f ? -30.f : (v > 30.f ? 30.f : v);
  return expf(v);
}

// The frame's output row (P floats, from HBM) one frame ahead in registers: a frame used to begin with the dependent load of its own row --
// 2-3 us of HBM latency in front of a 17-19 us frame, 500 times per recursion.  (More than kDenRowRegs * kDenThreads pdfs: the kernels load the rest
// the old way.)
constexpr int kDenRowRegs = 8;
struct RowAhead {
  float v[kDenRowRegs];
  __device__ __forceinline__ void load(const float *yr, int P, int tid) {
#pragma unroll
    for (int i = 0; i < kDenRowRegs; i++) {
      const int p = tid + i * kDenThreads;
      v[i] = p < P ? yr[p] : 0.f;
    }
  }
};

// The sum over one row of a sliced-ELL table (ap: the lane's first arc, w: the slice's width, uniform over the wave), arcs in order.  A row is a chain
// of dependent-latency loads from L2: batches of eight, then four, then ONE batch for the last one to three arcs (indices clamped, the surplus terms
// replaced by exact zeros) -- "#pragma unroll 4" left up to three single loads behind every row, "#pragma unroll 8" up to seven (measured: slower).
// Acc: the accumulator.  float everywhere but the occupancy rows of den_backward_kernel: a by-pdf row holds arcs / pdfs terms (1 300 at 13 000 states
// and 40 pdfs), and their sequential float sum alone put a frame's occupancies up to 6e-6 from summing to 1 where the recursions' rows (the
// in- and out-degree, a handful of arcs) cost nothing -- measured on peaky outputs (tests/test_gpu_chain_hostile.py, docs/experiments.md r6-n).
template <class Acc = float, class Term>
__device__ __forceinline__ Acc sell_row_sum(const uint2 *ap, int w, Term term) {
  Acc acc = 0;
  int j = 0;
  for (; j + 8 <= w; j += 8) {
    uint2 a[8];
#pragma unroll
    for (int u = 0; u < 8; u++) a[u] = ap[(j + u) * 64];
#pragma unroll
    for (int u = 0; u < 8; u++) acc += term(a[u]);
  }
  if (j + 4 <= w) {
    uint2 a[4];
#pragma unroll
    for (int u = 0; u < 4; u++) a[u] = ap[(j + u) * 64];
#pragma unroll
    for (int u = 0; u < 4; u++) acc += term(a[u]);
    j += 4;
  }
  if (j < w) {
    uint2 a[3];
#pragma unroll
    for (int u = 0; u < 3; u++) a[u] = ap[min(j + u, w - 1) * 64];
#pragma unroll
    for (int u = 0; u < 3; u++) acc += (j + u < w) ? term(a[u]) : 0.f;
  }
  return acc;
}

}  // namespace
}  // namespace tdnnf
