// batchnorm.h -- trainer-internal interface of BatchNorm.  Which file implements what:
//   batchnorm.hip   the forward / backward finalize kernels (memo rows 0-4), the apply passes of the stand-alone entries, StoreStats and the
//                   derived test-mode scale / offset, the thread-local BnSyncScope and FroBoundScope, batchnorm_stats*, tdnnf_batchnorm_*
//   fused.hip       the trainer's fused passes: bn_apply_bypass (forward), bn_relu_bwd (backward, with its own five-sum finalize)
//   this header     bn_finalize_synced: "finalize, with the collective in between" for all three finalize launches
#pragma once
#include "colreduce.h"

namespace tdnnf {

// Synchronised BatchNorm (data-parallel training): while one of these is installed, every train-mode BatchNorm of the calling thread
// all-reduces its column sums over the ranks -- forward [sum x, sum x^2], backward [sum z dz, sum dz, sum dz^2] (2 D / 3 D doubles
// in `buf`) -- through the caller's collective `fn(ctx, buf, count, stream)` before it forms mean / scale and the backward terms
// with the GLOBAL row count, so that a sharded minibatch normalises exactly as the whole one does
// (/root/reference/src/nnet3/nnet-normalize-component.cc:433-445 takes its statistics over all rows of the minibatch).
struct BnSync {
  int (*fn)(void *ctx, double *buf, long long count, tdnnf_stream stream);
  void *ctx;
  double *buf;      // device, >= 5 * max D doubles (the fused BatchNorm / ReLU backward stages five column sums, three are reduced)
  int world;
};
BnSync *bn_sync_current();
struct BnSyncScope {
  BnSync *prev;
  explicit BnSyncScope(BnSync *b);
  ~BnSyncScope();
};

// One finalize step: launch(sums_out, sums_in, N) starts the finalize kernel over N rows.  Without a BnSync that is one launch; with one,
// a launch that only leaves the column sums in sy->buf, the collective over the first `nsums` x D of them, and a launch that takes the
// sums from there with the global row count.
template <class Launch>
__attribute__((visibility("hidden"))) inline hipError_t bn_finalize_synced(BnSync *sy, int nsums, int D, int rows, hipStream_t s, Launch launch) {
  if (!sy) {
    launch((double *)nullptr, (const double *)nullptr, rows);
    return hipGetLastError();
  }
  launch(sy->buf, (const double *)nullptr, rows);
  if (sy->fn(sy->ctx, sy->buf, (long long)nsums * D, (tdnnf_stream)s)) return hipErrorUnknown;
  launch((double *)nullptr, (const double *)sy->buf, rows * sy->world);
  return hipGetLastError();
}

// While one of these is installed, the BatchNorm finalize launches of the calling thread -- the forward statistics (memo rows 0-2) and the
// backward terms of the fused BatchNorm / ReLU sweep -- also write, per block of kFinCols columns, an UPPER BOUND of the squared Frobenius
// norm of what the pass behind them produces (forward: z = (x - mean) scale, whose column sums of squares are N scale^2 var exactly;
// backward: the ReLU's input derivative, bounded by the column sums of squares of its output derivative, which the finalize forms
// anyway, plus the self-repair term).  planes_split takes its scale from such a bound instead of a pass over the matrix.
// buf: >= finalize_grid(D) doubles; *blocks receives how many were written (0: none -- test-mode BatchNorm has no such bound).
struct FroBoundScope {
  double *prev_buf;
  int *prev_blocks;
  FroBoundScope(double *buf, int *blocks);
  ~FroBoundScope();
};
double *fro_bound_buf();
int *fro_bound_blocks();

// BatchNorm forward: memo rows 0-2 from column partial sums / sums of squares laid out as colreduce_partial_into's with sq_row_offset == chunks
// store_stats (optional): BatchNormComponent::StoreStats ([count, sum[D], sumsq[D]] doubles += this minibatch) in the same launch
hipError_t batchnorm_stats_from_partials(const float *partial, int chunks, int rows, int cols, float epsilon, float target_rms, float *memo, hipStream_t s,
                                         double *store_stats = nullptr);
// the same from the matrix (both stages; the trainer applies the statistics in a fused pass, fused.hip); ws: colreduce_bytes(rows, cols)
hipError_t batchnorm_stats(MatView a, float epsilon, float target_rms, float *memo, void *ws, hipStream_t s, double *store_stats = nullptr);

}  // namespace tdnnf
