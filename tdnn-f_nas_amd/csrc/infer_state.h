// infer_state.h -- the whole-utterance inference object (tdnnf_infer, include/tdnnf_hip.h "inference") for its two units: infer.hip (the
// entries, the chunk plan, a batch's input and buffer description, the exact-f32 pass) and infer_planes.hip (the f16x3 pass on the plane
// kernels).  Both passes walk the one schedule of infer_forward.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "common.h"
#include "infer_forward.h"
#include "net_model.h"

namespace tdnnf {
struct InferPlanes;  // infer_planes.hip: weight planes, activation planes and scale records of an f16x3 object
}

struct tdnnf_infer {
  const tdnnf_net *model;
  int F, Tout, fsf, max_chunks, which;
  std::vector<tdnnf::TdnnfLayer> layers;  // grids at chunk width F (component ids from the model)
  tdnnf::Grid g_lda, g_feat;
  int nbn;
  tdnnf::BnTable bn;
  char *arena = nullptr;
  float *lda_in, *lda_out, *act[2], *lin, *lin_perm, *relu_tmp;
  tdnnf::FwdHead head;
  tdnnf::FwdBuffers fwd;  // where a batch of fwd_B chunks lives (infer_buffers)
  int fwd_B = 0;
  int *table = nullptr;  // device chunk table of the last compute
  size_t table_cap = 0;  // (ints)
  std::vector<int> host_table;
  int fused = 0, fallback = 0;
  tdnnf::InferPlanes *planes = nullptr;  // f16x3 objects only (tdnnf_infer_create_arith, gemm_precision 3)
  long long plane_gemms = 0, f32_gemms = 0;  // GEMM launches of the last compute (tdnnf_infer_gemm_counts)
};

namespace tdnnf {

// infer.hip: the batch's spliced lda input (q->lda_in, N0 x lda_dim) and its row map (q->head.row_map) from the chunk table entries at `tab`;
// the description of the buffers of a batch of B chunks, for either pass
int infer_batch_input(tdnnf_infer *q, const tdnnf_mat *feats, const tdnnf_mat *iv, const int *tab, int B, hipStream_t s);
const FwdBuffers &infer_buffers(tdnnf_infer *q, int B);

// infer_planes.hip.  create: the plane buffers of an object whose layers and buffers are laid out (q->planes); begin: the split of the
// weights of the chosen head's path, at the top of every compute; forward: one batch of B chunks whose input is in place (infer_batch_input), GEMM counts added to q's.
int infer_planes_create(tdnnf_infer *q);
void infer_planes_destroy(InferPlanes *p);
int infer_planes_begin(tdnnf_infer *q, hipStream_t s);
int infer_planes_forward(tdnnf_infer *q, int B, tdnnf_mat *out, hipStream_t s, FwdCounts *counts);

}  // namespace tdnnf
