// colreduce.h -- the two-stage deterministic column reduction.  Which file implements what:
//   colreduce.hip   first stage (colreduce_kernel: partial[quantity][chunk][col]), its plan and workspace size, the column-sum second
//                   stage (colsum_finalize) and colsum_add
//   this header     the second stage's block shape (kFin*) and finalize_sums, which every finalize kernel is built on: BatchNorm forward
//                   and backward (batchnorm.hip), the fused BatchNorm / ReLU backward (fused.hip), the column sum (colreduce.hip)
// Callers: rows_gemm.hip (tail rows of the statistics out of the GEMM epilogue), wgrad.hip (bias gradient), fused.hip, net_step.hip.
#pragma once
#include "common.h"

namespace tdnnf {

// Second stage of the column reductions: a 256-thread block owns 8 columns, its 32 lanes per column walk the partial rows
// four requests deep, then lane 0 adds the lanes' sums in a fixed order (deterministic).  The partial rows are few MB at most,
// the stage is pure latency: with 4 lanes x 24 blocks it took 45-300 us per call, ~5 ms per training step.  Rounds 2-4 ran it as
// 1024-thread blocks of 32 columns: beside another stream's kernels such a block waits until one CU has sixteen free wave slots at once
// (the BatchNorm finalize of the xent head beside the denominator and the statistics passes: 9 us alone, 234 us on average, 4.3 ms
// at worst in the round-5 trace); four-wave blocks fit wherever anything fits, and there are four times as many of them.
constexpr int kFinCols = 8, kFinLanes = 32, kFinThreads = kFinCols * kFinLanes;
inline unsigned finalize_grid(int D) { return (unsigned)((D + kFinCols - 1) / kFinCols); }
#ifdef __HIPCC__
// q[k] = sum over c < chunks of partial[((long long)k * qstride_rows + c) * D + d] for the calling thread's column d;
// valid afterwards in the threads with (threadIdx.x >> 5) == 0.  red: NQ * kFinLanes * (kFinCols + 1) elements of Acc.
template <int NQ, class Acc>
__device__ __forceinline__ void finalize_sums(const float *partial, int chunks, long long qstride_rows, int D, int nq, Acc (&q)[NQ], Acc *red) {
  const int tc = threadIdx.x & (kFinCols - 1), lane = threadIdx.x / kFinCols, d = blockIdx.x * kFinCols + tc;
#pragma unroll
  for (int k = 0; k < NQ; k++) q[k] = 0;
  if (d < D) {
    // (the NQ quantities side by side: their loads of a round are issued together -- one after the other, five quantities took 15 us
    // where two took 5)
    const float *p = partial + d;
    const long long qs = qstride_rows * D;
    int c = lane;
    for (; c + 3 * kFinLanes < chunks; c += 4 * kFinLanes) {
      float v[NQ][4];
#pragma unroll
      for (int k = 0; k < NQ; k++) {
        if (k < nq) {
          const float *pk = p + (long long)k * qs;
          v[k][0] = pk[(long long)c * D]; v[k][1] = pk[(long long)(c + kFinLanes) * D];
          v[k][2] = pk[(long long)(c + 2 * kFinLanes) * D]; v[k][3] = pk[(long long)(c + 3 * kFinLanes) * D];
        }
      }
#pragma unroll
      for (int k = 0; k < NQ; k++) {
        if (k < nq) { q[k] += v[k][0]; q[k] += v[k][1]; q[k] += v[k][2]; q[k] += v[k][3]; }
      }
    }
    for (; c < chunks; c += kFinLanes) {
      float v[NQ];
#pragma unroll
      for (int k = 0; k < NQ; k++)
        if (k < nq) v[k] = p[(long long)k * qs + (long long)c * D];
#pragma unroll
      for (int k = 0; k < NQ; k++)
        if (k < nq) q[k] += v[k];
    }
  }
#pragma unroll
  for (int k = 0; k < NQ; k++) red[(k * kFinLanes + lane) * (kFinCols + 1) + tc] = q[k];
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NQ; k++) {
      Acc s = 0;
      for (int l = 0; l < kFinLanes; l++) s += red[(k * kFinLanes + l) * (kFinCols + 1) + tc];
      q[k] = s;
    }
  }
}
#endif

struct ColReducePlan {
  int chunks, rows_per_chunk;
};
ColReducePlan colreduce_plan(int rows, int cols);
size_t colreduce_bytes(int rows, int cols);
// partial[q][chunk][col] for q < nq; kind: 0 = (sum a), 1 = (sum a, sum a*a), 2 = (sum a*b, sum b), 3 = (sum a, sum a>0)
hipError_t colreduce_partial(int kind, MatView a, MatView b, float *partial, hipStream_t s);
// the same with the chunking given: partial[c * cols + col] and, second quantity, partial[(sq_row_offset + c) * cols + col], c < chunks
hipError_t colreduce_partial_into(int kind, MatView a, MatView b, int chunks, int rows_per_chunk, int sq_row_offset, float *partial, hipStream_t s);
// second stage of a column sum: acc[d] += scale * sum over r < rows_of_partials of partial[r * D + d]
__attribute__((visibility("hidden"))) hipError_t colsum_finalize(const float *partial, int rows_of_partials, int D, float scale, float *acc, hipStream_t s);
// acc[c] += scale * colsum(a)[c], both stages; ws: colreduce_bytes(rows, cols)
hipError_t colsum_add(MatView a, float scale, float *acc, void *ws, hipStream_t s);

}  // namespace tdnnf
