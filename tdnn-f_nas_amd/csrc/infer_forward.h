// infer_forward.h -- what the three forward-only passes share (infer_forward.hip): the whole-utterance inference in exact f32 (infer.hip) and
// in f16x3 (infer_planes.hip) and the streaming one (online.hip).  The schedule of a pass is written once, in infer_forward(); a reader
// describes where its matrices live (FwdBuffers) and which GEMM runs (FwdGemm).  Beside it: the model checks, the test-mode BatchNorm
// coefficients, the rows GEMM with the inference epilogue and the row-map scatter.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "common.h"
#include "net_model.h"

namespace tdnnf {

// the models forward-only inference supports (the 7q graph and derived children, exact f32) and its width rule; `who` names the entry
int infer_check_model(const tdnnf_net_config &c, int frames, const char *who, const char *frames_name);

// Test-mode BatchNorm of every stage from the model's statistics [count, sum[D], sumsq[D]]: block i of `coef` = [mean | variance |
// scale | offset] (D each; mean and scale where bn_apply_bypass reads them, offset = -mean * scale for the GEMM epilogue).
constexpr int kMaxBn = TDNNF_NET_MAX_LAYERS + 3;
struct BnTable {
  const double *stats[kMaxBn];
  int D[kMaxBn];
  long long coef_off[kMaxBn];
};
inline long long infer_bn_stride(const tdnnf_net_config &c) { return 4LL * ldpad(std::max(c.hidden_dim, c.prefinal_small_dim)); }
// the stages of one head's path in network order: tdnn1, the tdnnf layers, the head's two (the model's statistics, by reference)
int infer_bn_table(const tdnnf_net *model, int which_output, BnTable *bn);
// nbn blocks of infer_bn_stride floats into coef (read at every call: an update of the model is seen by the next one)
hipError_t infer_bn_coef(const BnTable &bn, int nbn, float *coef, hipStream_t s);

// the indexes of an affine layer: one tap at row 0, every row
tdnnf_tdnn_indexes one_tap();
// the two TdnnComponents of the model's layer l between a reader's grids (.linear: lin_in -> lin_out, .affine: aff_in -> aff_out) for B sequences
void layer_tdnns(const tdnnf_net *model, int l, const Grid &lin_in, const Grid &lin_out, const Grid &aff_in, const Grid &aff_out, int B, Tdnn *lin,
                 Tdnn *aff);

// rows GEMM of one TdnnComponent (or affine: ix = one tap) with the inference epilogue (RowsGemmArgs::col_scale / col_offset / post_add /
// row_map); with no coef, add and row_map it is the launch of tdnn_propagate_impl, whose argument checks it makes
int gemm_post(const tdnnf_tdnn_indexes &ix, const tdnnf_mat &in, const float *W, int ldw, int Do, int Di, const float *bias, int relu,
              const float *coef, const tdnnf_mat *add, float add_scale, const int *row_map, const tdnnf_mat &out, hipStream_t s);

// out[row_map[m]] = in[m] for the rows that have one (16-byte accesses where both views allow them)
hipError_t infer_scatter_rows(const MatView &in, const int *row_map, const MatView &out, hipStream_t s);

// the head's temporaries for at most No output rows (y, lsm: the xent head only), the row map and the nbn blocks of BatchNorm coefficients;
// own_b1: a reader with no free activation buffer for the head's affine; table_ints: a device table of the reader's own
struct FwdHead {
  float *pl, *b1, *b2, *y, *lsm, *coef;
  int *row_map, *table;
};
void infer_head_layout(const tdnnf_net_config &c, int which, int nbn, long long No, bool own_b1, size_t table_ints, Arena &A, FwdHead *h);

// ---- the schedule
//   spliced input -> lda -> tdnn1 (+ ReLU + BatchNorm in the epilogue)
//   per TDNN-F layer: .linear GEMM -> [row reorder] -> .affine GEMM with ReLU + BatchNorm + bypass in the epilogue, or (bypass rows strided
//       against the output rows) ReLU in the GEMM and bn_apply_bypass after it
//   head: prefinal-l -> affine (+ ReLU + batchnorm1) -> linear (+ batchnorm2) -> output through the row map | output, log-softmax, scatter
// Where one call's matrices live, for B sequences (filled by the reader; `layers` is sized once, at create):
struct FwdLayer {
  Tdnn lin, aff;
  tdnnf_mat lin_in, lin_out;  // the rows the .linear reads, where its GEMM stores
  tdnnf_mat perm_out;         // aff.ix.row_stride > 1: lin_out is then reordered into it (the rho row order the .affine reads)
  tdnnf_mat aff_in, byp, out;  // the rows the .affine reads, the input rows under the output rows, the layer's output
  tdnnf_mat relu;              // strided bypass (data non-null): the .affine + ReLU before bn_apply_bypass writes out_times time rows of `out`
  int out_times;
};
struct FwdBuffers {
  tdnnf_mat lda_in, lda_out, x0;  // spliced input, lda output, tdnn1's output
  std::vector<FwdLayer> layers;
  tdnnf_mat top, pl, b1, b2, y, lsm;  // the head's input and temporaries (y, lsm: the xent head only)
  const int *row_map;
};
// One GEMM of the schedule.  role: 0 lda, 1 tdnn1, 2 + 2 l / 3 + 2 l layer l's .linear / .affine, then prefinal-l and the head's affine,
// linear, output; comp: its component of the model.  wants_stats: the next GEMM reads `out` (a plane GEMM then leaves its sums of squares).
typedef int (*FwdGemm)(void *ctx, hipStream_t s, int role, int comp, const tdnnf_tdnn_indexes &ix, const tdnnf_mat &in, int relu, const float *coef,
                       const tdnnf_mat *add, float add_scale, const int *row_map, const tdnnf_mat &out, bool wants_stats);
struct FwdCounts {
  int fused, fallback;    // stages whose BatchNorm rode on their GEMM / layers that took the bn_apply_bypass pass
  long long gemms, rows;  // GEMM calls and the sum of their output rows
};
// coef: the blocks of infer_bn_coef; which: the head; out: the caller's stacked output (the row map's target)
int infer_forward(const tdnnf_net *model, const float *coef, int which, int B, const FwdBuffers &b, tdnnf_mat *out, FwdGemm gemm, void *ctx,
                  hipStream_t s, FwdCounts *counts);
// the exact-f32 FwdGemm: gemm_post on the model's parameters (ctx: the model)
int infer_gemm_f32(void *ctx, hipStream_t s, int role, int comp, const tdnnf_tdnn_indexes &ix, const tdnnf_mat &in, int relu, const float *coef,
                   const tdnnf_mat *add, float add_scale, const int *row_map, const tdnnf_mat &out, bool wants_stats);

}  // namespace tdnnf
