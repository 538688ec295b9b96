// infer_parts.h -- what the whole-utterance inference (infer.hip, which defines all of it) shares with the streaming one (online.hip):
// the model checks, the test-mode BatchNorm coefficients, the rows GEMM with the inference epilogue and the row-map scatter.
#pragma once
#include <hip/hip_runtime.h>

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

// rows GEMM of one TdnnComponent (or affine: ix = one tap) with the inference epilogue (RowsGemmArgs::col_scale / col_offset / post_add / row_map)
int gemm_post(const tdnnf_tdnn_indexes &ix, const tdnnf_mat &in, const float *W, int ldw, int Do, int Di, const float *bias, int relu,
              const float *coef, const tdnnf_mat *add, float add_scale, const int *row_map, const tdnnf_mat &out, hipStream_t s);

// out[row_map[m]] = in[m] for the rows that have one (16-byte accesses where both views allow them)
hipError_t infer_scatter_rows(const MatView &in, const int *row_map, const MatView &out, hipStream_t s);

}  // namespace tdnnf
