// net.h -- data structures of the chain trainer, shared with the model reader / writer (model_io.hip) and the forward-only inference
// (infer_forward.hip and its readers).  What the model IS (statistics blocks, ranks, component walk, taps, head names) is described once, in net_model.h.
//
// File map of the trainer's net object:
//   net_model.h     the one description of the model that the units below, net_step.hip, model_io.hip and the inference read
//   net_graph.hip   host only, no HIP call: config checks, time grids, TdnnComponent indexes, the component list with its draw plan,
//                   cv-update factors, the "same model" check, gradient-bucket ranges, and the lists net_model.h declares
//   net_arena.hip   the arena layout as a sequence of named parts (sizing pass and real pass run the same function), named activations
//   net_create.hip  create (describe, allocate, name) / destroy, the streams and events of the first step, accessors and setters, the
//                   statistics get / set
//   net_update.hip  the optimizer step (tdnnf_net_update) with transpose_kernel and scale_doubles_kernel
//   net_step.h      one minibatch (forward, chain objective, backward) as one object, Step, with the map of its units: net_step.hip the
//                   schedule, net_step_planes.hip the plane operands, net_step_grad.hip gradients and natural-gradient scheduling,
//                   net_supernet.hip the supernets' ops
//   splice.hip      tdnnf_splice_input / tdnnf_reorder_rows with their kernels (no net object)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include <map>

#include "batchnorm.h"
#include "common.h"
#include "planes_gemm.h"
#include "tdnnf_hip.h"

namespace tdnnf {
struct RowsGemmGroup;  // gemm_f32.h
struct PlanesSplitGroup;  // planes_gemm.h

struct NgGroup;
struct NgFin;
struct UpdGroup;

struct Grid {
  int t0, step, n;
  int last() const { return t0 + step * (n - 1); }
};

struct CompDesc {
  std::string name;
  long long begin;
  int rows, cols, has_bias;
  float lr_factor, l2, max_change, orthonormal;
  int num_alpha;  // DARTS: K architecture logits between the weights and the bias
  bool plain = false;  // updated without natural gradient (OnehotFunction / ConstantFunction output_ vectors)
  bool updatable = true;  // false: the fixed lda layer (FixedAffineComponent: no learning-rate factor, never a gradient)
  long long size() const { return (long long)rows * cols + num_alpha + (has_bias ? rows : 0); }
};

struct Tdnn {  // one TdnnComponent instance inside the net
  int comp;    // index into comps
  int Di, Do, K;
  int offsets[TDNNF_MAX_OFFSETS];
  Grid in, out;
  // DARTS (TdnnDARTSV3Component): share index, first random draw, coefficient memo [coef(K) | eff(K)] on device
  bool darts;
  int share, draw0;
  float *memo;
  int *active;  // device: [count, tap ids...] of the non-zero taps (uniform-sample mode)
  tdnnf_tdnn_indexes ix;
  int rows_in, rows_out;
};
// the largest row shift of a component's taps (the lead rows of a backward-data view of its input)
inline int max_off(const Tdnn &td) {
  int m = 0;
  for (int i = 0; i < td.K; i++) m = std::max(m, td.ix.row_offsets[i]);
  return m;
}

struct TdnnfLayer {
  int stride, bn;
  int left, right;  // X.linear taps {-left, 0}, X.affine taps {0, right} (= stride unless the config gives layer offsets)
  Tdnn lin, aff;
  Grid gin, gout, glin;
  bool perm;  // affine input needs the rho row order
  int bypass_row0, bypass_rowstep;  // rows of the layer input that line up with the output grid
  // activations (arena)
  float *lin_out, *lin_perm, *relu_out, *noop_out;
  float *bn_memo;
  double *bn_stats, *relu_stats;
  // bottleneck-dimension supernet: component of the C-vector (X.softmax / X.alpha), first random draw, choice
  // probabilities p (C) and the column mask (bn), masked linear output
  int c_arch, arch_draw0;
  float *arch_p, *arch_mask, *lin_masked;
};

}  // namespace tdnnf

struct tdnnf_net {
  tdnnf_net_config cfg = {};
  std::vector<tdnnf::CompDesc> comps;
  long long num_params = 0;
  float *params = nullptr, *grads = nullptr;
  float *paramsT = nullptr;  // gemm_precision 1 / 2: per component, the transpose of its weight matrix at the same offset (backward-data GEMMs)
  // Pre-split plane operands (planes_gemm.h; gemm_precision 3 "f16x3", or 2 "bf16x6" with option planes): 0 = off, else planes per element.
  // Every matrix that is a GEMM operand has a slot (storage for its row-major and transposed planes and its scale), keyed by the
  // matrix's base pointer; a slot's CONTENT is only what the last split put there -- forward_backward() splits an operand where it is
  // produced and hands the description to the GEMM as a hint.  pw: the weight matrices' planes, re-split at the start of every step.
  int planes_np = 0;
  struct PlaneSlot {
    void *P = nullptr, *PT = nullptr;
    size_t bytesP = 0, bytesPT = 0;
    float *scale = nullptr;
    long long last[5] = {-1, -1, -1, -1, -1};  // (rows, cols, lead, R, layouts) of the last split: the same again leaves the zero rows as they are
  };
  std::map<const float *, PlaneSlot> plane_slots;
  std::vector<tdnnf::PlanesOperand> pw;  // by component
  std::vector<float *> pw_scale;         // their scale records
  void *planes_ws = nullptr;
  double *fro_buf = nullptr;  // FroBoundScope target: per-block norm bounds a BatchNorm finalize launch leaves for the next split (batchnorm.h)
  int B = 0, T = 0, Tout = 0;
  // graph
  tdnnf::Grid g_lda = {}, g_feat = {};
  tdnnf::Tdnn tdnn1 = {};  // affine 220 -> hidden on g_lda
  std::vector<tdnnf::TdnnfLayer> layers;
  int c_lda = 0, c_prefinal_l = 0;
  struct Head {
    int c_affine = 0, c_linear = 0, c_output = 0;
    float *aff_relu = nullptr, *bn1_out = nullptr, *lin_out = nullptr, *bn2_out = nullptr, *y = nullptr;
    float *bn1_memo = nullptr, *bn2_memo = nullptr;
    double *bn1_stats = nullptr, *bn2_stats = nullptr, *relu_stats = nullptr;
  } head[2];  // 0 chain, 1 xent (net_model.h head_name)
  float *xent_logsoftmax = nullptr;
  // arena
  char *arena = nullptr;
  size_t arena_bytes = 0;
  float *lda_in = nullptr, *lda_out = nullptr, *t1_relu = nullptr, *t1_bn = nullptr;
  float *t1_bn_memo = nullptr;
  double *t1_bn_stats = nullptr, *t1_relu_stats = nullptr;
  float *prefinal_l_out = nullptr;
  float *dA = nullptr, *dB = nullptr, *dC = nullptr, *d_small = nullptr, *d_small2 = nullptr;  // derivative scratch
  float *d_y = nullptr, *d_xent = nullptr;
  float *tapgrad = nullptr;      // DARTS: unscaled per-tap weight gradients (Do x K*Di) of the component being processed
  double *tapdots = nullptr;     // DARTS: s_i = <dW_i, W_i>
  const float *draws = nullptr;  // DARTS: uniform draws of this step (caller-owned device buffer)
  std::vector<tdnnf_ng *> ng_in, ng_out;  // per component (natural gradient)
  float *orthoT = nullptr;       // transpose of a constrained matrix with more rows than columns (null when there is none)
  // Natural gradient.  Per component the N-sized passes (raw gradient into T, H = X W^T either side, J on a refresh) run on the
  // caller's stream (or the weight-gradient stream) into buffers the component keeps for the step; everything latency-bound that
  // follows (L, traces, the rank-R projections of T, commit; K and the host hand-off on a refresh) runs ONCE PER GRADIENT BUCKET
  // as grouped launches on stream s3 (ng.h, ng_group.hip).  The per-object form of that chain remains for the first minibatch
  // (the preconditioners initialise themselves from it) and for option ng_grouped = 0.
  struct NgComp {
    float *H_in = nullptr, *H_out = nullptr, *T = nullptr, *bsum = nullptr;
    double *part_in = nullptr, *part_out = nullptr;
    int N = 0;
  };
  std::vector<NgComp> ngc;         // by component
  float *ng_bsum_all = nullptr;    // the components' raw bias gradients (NgComp::bsum), one block: zeroed once per step
  size_t ng_bsum_floats = 0;
  float *ngTmp = nullptr;          // per-object chain: projection scratch
  void *ng_side_ws = nullptr;      // per-object chain: workspace of L = H^T H
  size_t ngset_ws_bytes = 0;
  struct NgBucket {
    int key;
    std::vector<int> comps;
    tdnnf::NgGroup *group;
  };
  std::vector<NgBucket> ng_buckets;  // created the first time a bucket closes with every preconditioner initialised
  std::vector<int> ng_cur;           // components enqueued since the last bucket closed
  tdnnf::NgFin *ngfin = nullptr;
  bool ng_grouped = true;
  hipEvent_t ev_ngc = nullptr;       // the components' N-sized passes of a bucket are enqueued
  hipStream_t s3 = nullptr;
  hipEvent_t ev_s3 = nullptr;
  hipEvent_t ev_fin0 = nullptr, ev_fin = nullptr;  // step start -> s3, and s3's refresh uploads -> the backward pass
  float *s3_scratch = nullptr;   // split-K scratch of the GEMMs launched on s3
  size_t s3_scratch_bytes = 0;
  // Weight-gradient stream: a component's parameter gradient (and, with natural gradient, the N-sized statistics passes) is
  // independent of the backward-data GEMM that follows it.  At the recipes' minibatch (3 200 rows) neither fills the chip, so
  // they run side by side: param_grad() goes to s4 with a workspace of its own, the caller's stream waits for the one before
  // the last (the buffers a gradient reads are rewritten two components later at the earliest).  Off for minibatches whose
  // GEMMs fill the chip by themselves (option wgrad_stream = 0 | 1 forces it).
  bool wg_on = false;
  hipStream_t s4 = nullptr;
  hipEvent_t ev_pg[4] = {nullptr, nullptr, nullptr, nullptr}, ev_pg_in = nullptr;
  int wg_lag = 3;        // the caller's stream waits for the weight gradient of the component wg_lag back (option wgrad_lag: 1 or 3)
  float *dC2 = nullptr, *dS[2] = {nullptr, nullptr};  // wg_lag 3: second buffers for the derivative matrices weight gradients read (net_step.hip)
  unsigned pg_count = 0;
  void *ws4 = nullptr;
  void *ws2 = nullptr;           // the same for components whose weight gradients go to the denominator's stream (wg_two)
  float *s2_scratch = nullptr;
  float *s4_scratch = nullptr;   // split-K scratch of the GEMMs launched on s4
  hipStream_t s5 = nullptr;  // option wgrad_stream 3: a third weight-gradient stream with its workspace and split-K scratch
  void *ws5 = nullptr;
  float *s5_scratch = nullptr;
  // Input-side natural-gradient statistics ahead of the backward pass: H_in = X~ W_x^T (and J = H^T X on refresh steps) of a component
  // needs its forward input and the preconditioner state only, so from the second grouped minibatch on they are launched on s4 as soon as
  // the forward pass is enqueued -- beside the denominator and the xent head, HBM-bound work beside MFMA-bound work -- with the
  // arguments the component's backward call recorded one minibatch earlier (early_rec), checked again when that call comes.
  struct EarlyIn {
    unsigned char xin[256];  // a tdnnf::NgInput (net.h does not see ng.h)
    long long recorded = -1, done = -1;  // fb_count values
  };
  std::vector<EarlyIn> early;
  long long fb_count = 0;
  bool early_on = false, early_any = false;
  bool early_group = false;                    // the early passes as ONE grouped launch on s4 (minibatches with the weight-gradient streams)
  tdnnf::RowsGemmGroup *early_launch = nullptr;  // its device-side task table
  tdnnf::PlanesSplitGroup *wsplit_group = nullptr;  // f16x3: the task table of the grouped split of a step's weight matrices
  hipEvent_t ev_early_in = nullptr, ev_early = nullptr;
  size_t s4_scratch_bytes = 0;
  bool wg_two = false;  // this step, from the denominator's join on: weight-gradient components alternate between s4 and s2
  float *gtmp = nullptr;         // this minibatch's gradient; committed into `grads` only when the objective was finite
  // NonlinearComponent::StoreBackpropStats skips a minibatch w.p. 1/4 only "&& oderiv_count_ != 0" (nnet-component-itf.cc:466): whether a
  // ReLU's oderiv_count is non-zero, by relu_index (net_model.h: the k-th ReLU of stat_blocks(); host copy: set by set_stats / read_model and by every store);
  // a net made by tdnnf_net_create_shared looks at the primary's
  std::vector<char> oderiv_nonzero_own;
  std::vector<char> *oderiv_nonzero = &oderiv_nonzero_own;
  tdnnf::BnSync bn_sync{nullptr, nullptr, nullptr, 1};  // tdnnf_net_set_batchnorm_sync; buf lives in the arena
  // diagnostics (option phase_events): events on the caller's stream at the phase boundaries of the last step
  enum { kPhases = 8 };  // 0 start, 1 forward trunk done, 2 heads forward + xent objective issued, 3 heads' backward done, 4 trunk backward done, 5 side streams joined, 6 update start, 7 update done
  hipEvent_t ev_phase[kPhases] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  bool phase_rec[kPhases] = {false, false, false, false, false, false, false, false};
  tdnnf::UpdGroup *upd = nullptr;  // the optimizer step's grouped launches (optim_group.h): built at the first update for the parameter buffer in use
  bool den_split = true;  // the denominator's two recursions side by side (option den_split, read when the net's first step sizes the workspace)
  hipStream_t s2 = nullptr;      // the denominator runs here, beside the xent head on the caller's stream
  hipEvent_t ev_fork = nullptr, ev_den = nullptr, ev_num = nullptr;  // ev_num: the numerator recursion (side stream) is done
  hipEvent_t ev_den_rec = nullptr;     // option xent_behind_den: the denominator's two recursions are done
  hipEvent_t ev_comm = nullptr;        // tdnnf_net_allreduce_grads_rccl: the last bucket's collective
  int num_draws = 0;
  bool owns_ng = true;    // false: created by tdnnf_net_create_shared, the preconditioners belong to the primary net
  int dropout_draw0 = 0;      // first of the (num_layers + 1) * B * hidden_dim dropout draws (cfg.use_dropout)
  float *dropout_masks = nullptr;   // (num_layers + 1) x B x hidden_dim: tdnn1, then the tdnnf layers
  float dropout_proportion = 0.f;
  void *ws = nullptr;
  size_t ws_bytes = 0;
  void *chain_ws = nullptr;
  size_t chain_ws_bytes = 0;
  std::vector<std::pair<std::string, tdnnf_mat>> named;
  // Gradient buckets for a data-parallel caller (tdnnf_net_grad_bucket): contiguous ranges of the flat gradient buffer in the
  // order the backward pass finishes them; `ready` is recorded once the range is final in `grads`
  struct GradBucket {
    long long begin, end;
    int close_key;  // closed after: -2 prefinal-l (heads + prefinal-l), l >= 0 tdnnf layer l, -1 tdnn1 (the rest)
    hipEvent_t ready = nullptr, handoff = nullptr;  // (created with the net's other resources, net_create.hip)
  };
  std::vector<GradBucket> buckets;
  // debugging / parity (tdnnf_net_set_capture): copies of the backward pass's derivative matrices, which live in recycled
  // scratch buffers, kept under names ("tdnnf5.affine.deriv", ...) that tdnnf_net_get_activation serves
  bool capture_on = false;
  std::vector<float *> captured;
};

namespace tdnnf {
// parameter / gradient views of component `comp` inside the flat buffers
inline float *net_W(const tdnnf_net *n, int comp) { return n->params + n->comps[comp].begin; }
inline float *net_alpha(const tdnnf_net *n, int comp) {
  const CompDesc &c = n->comps[comp];
  return c.num_alpha ? n->params + c.begin + (long long)c.rows * c.cols : nullptr;
}
inline float *net_bias(const tdnnf_net *n, int comp) {
  const CompDesc &c = n->comps[comp];
  return c.has_bias ? n->params + c.begin + (long long)c.rows * c.cols + c.num_alpha : nullptr;
}
// the same places in this minibatch's gradient (gtmp); net_Ag: the architecture logits' (whatever num_alpha is)
inline float *net_Wg(const tdnnf_net *n, int comp) { return n->gtmp + n->comps[comp].begin; }
inline float *net_Ag(const tdnnf_net *n, int comp) { return n->gtmp + n->comps[comp].begin + (long long)n->comps[comp].rows * n->comps[comp].cols; }
inline float *net_Bg(const tdnnf_net *n, int comp) {
  const CompDesc &c = n->comps[comp];
  return c.has_bias ? n->gtmp + c.begin + (long long)c.rows * c.cols + c.num_alpha : nullptr;
}
// Row stride of every activation matrix of the trainer: a multiple of 32 floats, so that rows start on 128-byte lines.
// (With the 16-byte minimum, the 6034-wide output matrices ran their GEMMs at 80 instead of 120 TFLOP/s: every 128-byte
// row segment a tile load fetches straddled two cache lines.)
inline int ldpad(int cols) { return (cols + 31) & ~31; }
inline tdnnf_mat M(float *p, int rows, int cols) { return tdnnf_mat{p, rows, cols, ldpad(cols)}; }
inline int N_of(const Grid &g, int B) { return g.n * B; }
// Bump allocator over one device allocation, 256-byte aligned; with base == nullptr it only sizes (take() returns null)
// (the reserved handles' Carve, assign_stage.h, is the same idea; it pads a zero-length piece to one element, this one must not: the net's layout stays)
struct Arena {
  size_t off = 0;
  char *base = nullptr;
  template <class T>
  T *take(size_t n) {
    off = (off + 255) & ~(size_t)255;
    T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
    off += sizeof(T) * n;
    return p;
  }
  float *mat(long long rows, int cols) { return take<float>((size_t)rows * ldpad(cols)); }
};
// net_arena.hip: carve (or size) every buffer of the net, latching the options that decide which exist (wg_lag, wg_on, early_on, early_group,
// ng_grouped, planes_np); the table of named activations that tdnnf_net_get_activation serves
void net_layout_arena(tdnnf_net *n, Arena &A);
void net_name_activations(tdnnf_net *n);
// net_create.hip: what the first step of a net creates (the chain workspace, the streams and events of the step, in a fixed order)
int create_streams_and_events(tdnnf_net *n, const tdnnf_den_graph *den);
// view of the rows of a t-major matrix (grid g, B sequences, `cols` wide) that lie on a coarser grid `sub`
inline tdnnf_mat sub_grid_view(float *data, const Grid &g, const Grid &sub, int B, int cols) {
  const int stride = ldpad(cols);
  const int tau0 = (sub.t0 - g.t0) / g.step, ratio = sub.step / g.step;
  if (ratio == 1) return tdnnf_mat{data + (size_t)tau0 * B * stride, sub.n * B, cols, stride};
  // every ratio-th block of B rows: n "super rows" of B*stride elements
  return tdnnf_mat{data + (size_t)tau0 * B * stride, sub.n, B * stride - (stride - cols), ratio * B * stride};
}
// diagnostics: phase boundary k of the step (option phase_events)
inline int phase_mark(tdnnf_net *n, int k, hipStream_t s) {
  if (!options().phase_events) return TDNNF_OK;
  if (!n->ev_phase[k]) TDNNF_HIP(hipEventCreate(&n->ev_phase[k]));
  TDNNF_HIP(hipEventRecord(n->ev_phase[k], s));
  n->phase_rec[k] = true;
  return TDNNF_OK;
}
}  // namespace tdnnf

#define CK(expr)             \
  do {                       \
    int rc__ = (expr);       \
    if (rc__) return rc__;   \
  } while (0)
