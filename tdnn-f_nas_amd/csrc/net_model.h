// net_model.h -- the one description of the model behind a tdnnf_net, for its four readers: the net's own units (net_graph.hip,
// net_arena.hip, net_create.hip, net_update.hip), the step (net_step.hip), the model reader / writer (model_io.hip) and the
// forward-only inference (infer_forward.hip: the one schedule; infer.hip, infer_planes.hip, online.hip: its three readers).  Whoever adds a statistics block, a component kind or a head changes THIS file and net_graph.hip.
#pragma once
#include <string>
#include <vector>

#include "net.h"

namespace tdnnf {

// ---- heads: 0 "chain", 1 "xent" (prefinal-<name>.*; the outputs are "output" and "output-xent")
inline const char *head_name(int h) {
  static const char *const names[2] = {"chain", "xent"};
  return names[h];
}

// ---- BatchNorm / ReLU statistics outside the parameter vector (doubles, on the device)
//   BatchNorm  [count, sum[D], sumsq[D]]
//   ReLU       [count, value_sum[D], deriv_sum[D], oderiv_count, oderiv_sumsq[D]]
//   memo of a BatchNorm (floats): five D-vectors (batchnorm.hip)
inline int bn_stats_doubles(int D) { return 1 + 2 * D; }
inline int relu_stats_doubles(int D) { return 2 + 3 * D; }
inline int relu_oderiv_at(int D) { return 1 + 2 * D; }  // offset of oderiv_count; oderiv_sumsq follows it
inline int bn_memo_floats(int D) { return 5 * D; }
// The statistics blocks of a net in network order -- the order of tdnnf_net_get_stats / _set_stats and of the arena:
//   tdnn1 (batchnorm, relu), every tdnnf layer (batchnorm, relu), both heads (batchnorm1, relu, batchnorm2).
// relu_index (net_step.hip Step::oderiv_of, tdnnf_net::oderiv_nonzero): the k-th ReLU block of this list, i.e. 0 tdnn1, 1 + l tdnnf
// layer l, num_layers + 1 + h head h.
struct StatBlock {
  std::string name;  // the component's name in a model file ("tdnn1.batchnorm", "prefinal-xent.relu", ...)
  double **slot;     // the net's pointer to the block (written only where a shared net adopts the primary's blocks)
  int D;
  bool relu;
  int head;          // -1 trunk, else the head the block belongs to
  double *p() const { return *slot; }
  int doubles() const { return relu ? relu_stats_doubles(D) : bn_stats_doubles(D); }
};
std::vector<StatBlock> stat_blocks(const tdnnf_net *n);

// ---- natural gradient: ranks of a component's input- and output-side preconditioners and their configuration
// (TdnnDARTSV3Component::InitFromConfig, nnet-tdnn-component.cc:183-210; the defaults of NaturalGradientAffineComponent / LinearComponent)
constexpr int kNgUpdatePeriod = 4;
constexpr float kNgNumSamplesHistory = 2000.0f;
constexpr float kNgAlpha = 4.0f;
inline void ng_ranks(const CompDesc &cd, int *rank_in, int *rank_out) {
  const int spliced = cd.cols + (cd.has_bias ? 1 : 0);
  *rank_in = std::min(20, (spliced + 1) / 2);
  *rank_out = std::min(80, (cd.rows + 1) / 2);
}

// ---- the weight components in network order: tdnn1, each layer's .linear and .affine, prefinal-l, both heads' affine / linear / output
struct WeightComp {
  int comp, K, rows_out;  // index into comps, taps, rows (N) of the output grid
};
std::vector<WeightComp> weight_comps(const tdnnf_net *n);

// ---- time grids (they replace the nnet3 compiler for these graphs)
// the grids of every tdnnf layer for Tout output frames (stride, taps, bottleneck, gout / glin / gin, perm), derived backwards from the
// output grid; *g_lda = the first layer's input grid
int net_layer_grids(const tdnnf_net_config &c, int Tout, std::vector<TdnnfLayer> &layers, Grid *g_lda);
// the feature frames under g_lda (which must run at the input frame rate, step 1): one more frame either side for the lda splice
inline Grid feat_grid(const Grid &g_lda) { return Grid{g_lda.t0 - 1, 1, g_lda.n + 2}; }
// the taps of a layer's .linear and .affine: the offset supernet's K at the input frame rate, else {-left, 0} / {0, right}, a zero
// offset leaving a single tap ("time-offsets=0", composite_layers.py:145-150, generate_top_list.py:109-118)
void layer_taps(const tdnnf_net_config &c, const TdnnfLayer &L, std::vector<int> *lin, std::vector<int> *aff);
// the indexes of one TdnnComponent between two grids for B sequences (t-major rows)
void make_tdnn(Tdnn *t, int comp, int Di, int Do, const std::vector<int> &offs, const Grid &in, const Grid &out, int B);

// ---- net_graph.hip for net_create.hip: what tdnnf_net_create checks and derives from the configuration without touching the device
int net_check_config(const tdnnf_net_config &c);
int net_describe(tdnnf_net *n);  // n->cfg -> B / T / Tout, grids, layers, components, draw plan, cv-update factors, gradient-bucket ranges
int net_same_model(const tdnnf_net *n, const tdnnf_net *primary);

}  // namespace tdnnf
