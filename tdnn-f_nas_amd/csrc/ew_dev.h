// ew_dev.h -- device helpers of the HBM-bound units (colreduce.hip, batchnorm.hip, elementwise.hip, log_softmax.hip, darts_ops.hip,
// fused.hip).  No __global__ function lives here: a kernel in a shared header is emitted by every unit that includes it, launched or not
// (docs/experiments.md r6-g).
//   ld / st                       four floats of a row as one float4, or the first of them as a scalar
//   ld4_ragged / st4_ragged       the float4 at column c of a row whose width is no multiple of four
//   wave_sum / wave_max, block_sum256 / block_max256   the fixed-order reductions of a 256-thread block
//   gumbel, softmax_short_row, onehot_bucket           the DARTS mixing arithmetic
#pragma once
#include "common.h"

namespace tdnnf {

__device__ __forceinline__ void ld(const float *p, float (&v)[4], bool vec) {
  if (vec) {
    const float4 t = *reinterpret_cast<const float4 *>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = p[0];
  }
}
__device__ __forceinline__ void st(float *p, const float (&v)[4], bool vec) {
  if (vec) *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else p[0] = v[0];
}

// columns c .. c + 3 (c % 4 == 0, c < cols) of a 16-byte aligned row of `cols` floats: one float4 where the row holds all four, else the
// one to three that exist (the load leaves the others of v as they are)
__device__ __forceinline__ void ld4_ragged(const float *row, int c, int cols, float4 &v) {
  if (c + 3 < cols) v = *reinterpret_cast<const float4 *>(row + c);
  else {
    v.x = row[c];
    if (c + 1 < cols) v.y = row[c + 1];
    if (c + 2 < cols) v.z = row[c + 2];
  }
}
// the store of f(v.x) .. f(v.w) to the same columns (f is evaluated only for the columns that exist)
template <class F>
__device__ __forceinline__ void st4_ragged(float *row, int c, int cols, const float4 v, F f) {
  if (c + 3 < cols) *reinterpret_cast<float4 *>(row + c) = make_float4(f(v.x), f(v.y), f(v.z), f(v.w));
  else {
    row[c] = f(v.x);
    if (c + 1 < cols) row[c + 1] = f(v.y);
    if (c + 2 < cols) row[c + 2] = f(v.z);
  }
}
__device__ __forceinline__ void st4_ragged(float *row, int c, int cols, const float4 v) {
  st4_ragged(row, c, cols, v, [](float x) { return x; });
}

__device__ __forceinline__ float wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// Sum / max over a block of 256 threads in a fixed order: wave shuffle, one value per wave in red[4], ONE barrier, then the four in the
// order written here.  A caller that uses `red` again puts its own barrier behind the call.
template <class T>
__device__ __forceinline__ T block_sum256(T v, T *red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ float block_max256(float v, float *red) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__device__ __forceinline__ float gumbel(float u) { return -logf(-logf(u)); }

// softmax over a short row v[0 .. n) in place (registers or global memory): max, exp(x - max), their sum in index order, the quotient,
// floored at 1e-20 the way ApplyFloor does
__device__ __forceinline__ void softmax_short_row(float *v, int n) {
  float mx = -INFINITY;
  for (int i = 0; i < n; i++) mx = fmaxf(mx, v[i]);
  float sum = 0.f;
  for (int i = 0; i < n; i++) sum += expf(v[i] - mx);
  for (int i = 0; i < n; i++) v[i] = floor_keep_nan(expf(v[i] - mx) / sum, 1.0e-20f);
}
// one-hot over C buckets of [0, 1): 1 for the bucket c that holds the draw u
__device__ __forceinline__ float onehot_bucket(float u, int c, int C) { return (u >= (float)c / C && u < (float)(c + 1) / C) ? 1.f : 0.f; }

}  // namespace tdnnf
