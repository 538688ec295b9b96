// colreduce.hip -- the two-stage deterministic column reduction (colreduce.h): sums down the columns of an N x D matrix, first per chunk of
// rows (colreduce_kernel), then over the chunks (a finalize kernel on finalize_sums; the plain column sum's is here, BatchNorm's are in
// batchnorm.hip and fused.hip).  Replaces the reference's AddRowSumMat / AddDiagMat2 / AddDiagMatMat chains.
#include "colreduce.h"
#include "ew_dev.h"

namespace tdnnf {
namespace {

// block = 64 float4-columns x 4 row lanes; each block reduces `rows_per_chunk` rows of 256 columns.
template <int KIND, int VEC>
__global__ __launch_bounds__(256) void colreduce_kernel(MatView a, MatView b, int rows_per_chunk, int chunks,
                                                        float *partial) {
  __shared__ float red[2][4][64 * 4 + 4];
  const int tc = threadIdx.x & 63, tr = threadIdx.x >> 6;
  const int col = (blockIdx.x * 64 + tc) * VEC;
  const int r0 = blockIdx.y * rows_per_chunk, r1 = min(a.rows, r0 + rows_per_chunk);
  float s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
  if (col < a.cols) {
    auto fetch = [&](int r, float (&va)[4], float (&vb)[4]) {
      if (VEC == 2) {  // (the 6034-wide output layer)
        float2 x = *reinterpret_cast<const float2 *>(a.data + (long long)r * a.stride + col);
        va[0] = x.x; va[1] = x.y;
        if (KIND == 2) {
          float2 y = *reinterpret_cast<const float2 *>(b.data + (long long)r * b.stride + col);
          vb[0] = y.x; vb[1] = y.y;
        }
      } else {
        ld(a.data + (long long)r * a.stride + col, va, VEC == 4);
        if (KIND == 2) ld(b.data + (long long)r * b.stride + col, vb, VEC == 4);
      }
    };
    auto add = [&](const float (&va)[4], const float (&vb)[4]) {
#pragma unroll
      for (int j = 0; j < VEC; j++) {
        if (KIND == 0) s0[j] += va[j];
        if (KIND == 1) { s0[j] += va[j]; s1[j] += va[j] * va[j]; }
        if (KIND == 2) { s0[j] += va[j] * vb[j]; s1[j] += vb[j]; }
        if (KIND == 3) { s0[j] += va[j]; s1[j] += va[j] > 0.f ? 1.f : 0.f; }
      }
    };
    int r = r0 + tr;
    for (; r + 12 < r1; r += 16) {  // four rows requested before the first is added: the pass is bound by requests in flight
      float va[4][4], vb[4][4];
#pragma unroll
      for (int u = 0; u < 4; u++) fetch(r + 4 * u, va[u], vb[u]);
#pragma unroll
      for (int u = 0; u < 4; u++) add(va[u], vb[u]);
    }
    for (; r < r1; r += 4) {
      float va[4], vb[4];
      fetch(r, va, vb);
      add(va, vb);
    }
  }
#pragma unroll
  for (int j = 0; j < VEC; j++) {
    red[0][tr][tc * VEC + j] = s0[j];
    red[1][tr][tc * VEC + j] = s1[j];
  }
  __syncthreads();
  if (tr == 0 && col < a.cols) {
#pragma unroll
    for (int j = 0; j < VEC; j++) {
      const float t0 = (red[0][0][tc * VEC + j] + red[0][1][tc * VEC + j]) + (red[0][2][tc * VEC + j] + red[0][3][tc * VEC + j]);
      const float t1 = (red[1][0][tc * VEC + j] + red[1][1][tc * VEC + j]) + (red[1][2][tc * VEC + j] + red[1][3][tc * VEC + j]);
      partial[(long long)blockIdx.y * a.cols + col + j] = t0;
      if (KIND != 0) partial[((long long)chunks + blockIdx.y) * a.cols + col + j] = t1;
    }
  }
}

// colsum finalize: acc[c] += scale * sum_chunks partial
__global__ __launch_bounds__(kFinThreads) void colsum_finalize_kernel(const float *partial, int chunks, int D, float scale, float *acc) {
  __shared__ float red[kFinLanes * (kFinCols + 1)];
  const int d = blockIdx.x * kFinCols + (threadIdx.x & (kFinCols - 1));
  float q[1];
  finalize_sums<1, float>(partial, chunks, chunks, D, 1, q, red);
  if (threadIdx.x < kFinCols && d < D) acc[d] += scale * q[0];
}

}  // namespace

ColReducePlan colreduce_plan(int rows, int cols) {
  ColReducePlan p;
  const int colblocks = (cols + 255) / 256;
  int chunks = (1024 + colblocks - 1) / colblocks;  // ~4 blocks per CU
  const int maxc = (rows + 31) / 32;
  if (chunks > maxc) chunks = maxc;
  if (chunks < 1) chunks = 1;
  p.rows_per_chunk = (rows + chunks - 1) / chunks;
  if (p.rows_per_chunk < 1) p.rows_per_chunk = 1;
  p.chunks = (rows + p.rows_per_chunk - 1) / p.rows_per_chunk;
  if (p.chunks < 1) p.chunks = 1;
  return p;
}
size_t colreduce_bytes(int rows, int cols) {
  ColReducePlan p = colreduce_plan(rows, cols);
  return sizeof(float) * 2 * (size_t)p.chunks * cols + 64;
}
hipError_t colreduce_partial(int kind, MatView a, MatView b, float *partial, hipStream_t s) {
  ColReducePlan p = colreduce_plan(a.rows, a.cols);
  return colreduce_partial_into(kind, a, b, p.chunks, p.rows_per_chunk, p.chunks, partial, s);
}
hipError_t colreduce_partial_into(int kind, MatView a, MatView b, int chunks, int rows_per_chunk, int sq_row_offset, float *partial, hipStream_t s) {
  const bool vec = vec4_ok(a) && (kind != 2 || vec4_ok(b));
  auto vec2_ok = [](const MatView &m) { return m.cols % 2 == 0 && m.stride % 2 == 0 && (reinterpret_cast<uintptr_t>(m.data) & 7) == 0; };
  const bool vec2 = !vec && vec2_ok(a) && (kind != 2 || vec2_ok(b));  // e.g. the 6034-wide output layer
  const int per = vec ? 256 : (vec2 ? 128 : 64);
  dim3 grid((a.cols + per - 1) / per, chunks), block(256);
#define CR(K)                                                                                              \
  if (vec) hipLaunchKernelGGL((colreduce_kernel<K, 4>), grid, block, 0, s, a, b, rows_per_chunk, sq_row_offset, partial); \
  else if (vec2) hipLaunchKernelGGL((colreduce_kernel<K, 2>), grid, block, 0, s, a, b, rows_per_chunk, sq_row_offset, partial); \
  else hipLaunchKernelGGL((colreduce_kernel<K, 1>), grid, block, 0, s, a, b, rows_per_chunk, sq_row_offset, partial);
  switch (kind) {
    case 0: CR(0) break;
    case 1: CR(1) break;
    case 2: CR(2) break;
    default: CR(3) break;
  }
#undef CR
  return hipGetLastError();
}

hipError_t colsum_finalize(const float *partial, int rows_of_partials, int D, float scale, float *acc, hipStream_t s) {
  hipLaunchKernelGGL(colsum_finalize_kernel, dim3(finalize_grid(D)), dim3(kFinThreads), 0, s, partial, rows_of_partials, D, scale, acc);
  return hipGetLastError();
}
hipError_t colsum_add(MatView a, float scale, float *acc, void *ws, hipStream_t s) {
  hipError_t e = colreduce_partial(0, a, a, (float *)ws, s);
  if (e != hipSuccess) return e;
  return colsum_finalize((const float *)ws, colreduce_plan(a.rows, a.cols).chunks, a.cols, scale, acc, s);
}

}  // namespace tdnnf

extern "C" {

size_t tdnnf_colreduce_workspace_bytes(int rows, int cols) { return tdnnf::colreduce_bytes(rows, cols); }

}  // extern "C"
