// net_step.h -- one minibatch of nnet3-chain-train on a tdnnf_net (net.h) as one object: Step.  Its members are the state that lives for one
// minibatch, its methods the pieces of the schedule; state that lives across minibatches stays in tdnnf_net.
//
// File map of the step:
//   net_step.hip         the schedule, top to bottom: run / run_objective, begin, the forward and backward phases with fork_objective*, join,
//                        the C entries; ahead of them the BatchNorm and affine helpers the phases call (bn_test_memo_kernel, dropout_mask_kernel)
//   net_step_planes.hip  plane operands (planes_gemm.h): the slot of a matrix, split, the weights' planes, the fused writers' descriptions;
//                        transpose_weights with its kernel
//   net_step_grad.hip    a component's gradient: param_grad / tdnn_wgrad, the choice of the weight-gradient stream and its event ring, the
//                        gradient buckets (commit_grads_kernel, the two tap-scaling kernels); the natural-gradient scheduling: refresh uploads,
//                        the early input-side statistics, the fused output-side statistic, the grouped chain of a bucket
//   net_supernet.hip     the ops of the two supernets behind three host functions (below): DARTS tap coefficients, the bottleneck choice
//   net_create.hip       create_streams_and_events (net.h): the first step of a net creates what tdnnf_net_destroy takes apart
#pragma once
#include <string.h>

#include <string>
#include <vector>

#include "batchnorm.h"
#include "common.h"
#include "fused.h"
#include "gemm_f32.h"
#include "net_model.h"
#include "ng.h"

#define TDNNF_STEP_LOCAL __attribute__((visibility("hidden")))  // shared between the units of the step only

namespace tdnnf {
// plane operands: split a matrix into its slot and describe it
enum { kP = 1, kT = 2 };
// (optional) norm bound a BatchNorm finalize launch left in n->fro_buf: blocks > 0 -> the split takes its scale from it (planes_gemm.h)
struct FroBound {
  int blocks = 0;
  float mul = 1.0f, add_coef = 0.0f;
  const float *add_rec = nullptr;
};
inline const PlanesOperand *hint_of(const PlanesOperand &o) { return o.base ? &o : nullptr; }
// a TdnnDARTSV3Component's effective tap coefficients (device: behind the K raw ones in its memo); null for a plain component
inline float *darts_eff(const Tdnn &td) { return td.darts ? td.memo + TDNNF_MAX_OFFSETS : nullptr; }

// net_supernet.hip.  TdnnDARTSV3Component::Propagate :250-289 for both components of the layer: the tap coefficients and the list of active taps
TDNNF_STEP_LOCAL int darts_coef(tdnnf_net *n, TdnnfLayer &L, hipStream_t s);
// bottleneck supernet: the choice probabilities and the column mask of this step, L.lin_masked = column blocks of L.lin_out times CopyN(Sum(p_k..))
TDNNF_STEP_LOCAL int bn_choice_forward(tdnnf_net *n, TdnnfLayer &L, hipStream_t s);
// d_lin is the derivative w.r.t. the masked blocks: the CopyN factor receives colsum(lin * d) (-> gradient of the C-vector), the linear
// output receives d * mask, in place (ElementwiseProductComponent::Backprop :276-299)
TDNNF_STEP_LOCAL int bn_choice_backward(tdnnf_net *n, TdnnfLayer &L, tdnnf_mat &d_lin, hipStream_t s);

struct TDNNF_STEP_LOCAL Step {
  // ---- the call
  tdnnf_net *const n;
  const tdnnf_mat *const feats, *const ivectors;
  const tdnnf_den_graph *const den;
  const tdnnf_supervision *const sup;
  double *const results;
  const long long step;
  const hipStream_t s;
  const int objective_flags;  // tdnnf_net_objective's flags; -1: a training step
  // ---- fixed for the step
  const tdnnf_net_config &c = n->cfg;
  const int B = n->B, Hd = c.hidden_dim, S = c.prefinal_small_dim, P = c.num_pdfs, lda_dim = 3 * c.feat_dim + c.ivector_dim;
  const int N0 = N_of(n->g_lda, B), No = n->Tout * B, np = n->planes_np, Ltop = c.num_layers - 1;
  const bool cv = c.cv_update != 0;  // BatchNorm components are BatchNormTestComponents
  const bool use_ng = c.use_natural_gradient != 0;
  // tdnnf_net_objective: the forward phases only, no state of the net touched but (with the flag, train mode) the BatchNorm statistics
  const bool objective = objective_flags >= 0;
  const bool store_bn = !objective || (objective_flags & TDNNF_OBJECTIVE_STORE_BATCHNORM_STATS) != 0;
  // (the weight-gradient stream reads operands while the caller's stream moves on: plane slots are reused per layer -- small minibatches keep the f32 kernels)
  const bool pl_on = np != 0 && !n->wg_on;
  // Weight gradients up to three components behind the caller's stream (option wgrad_lag, default 3; 1 = rounds 2-4: one behind).  A
  // buffer that component k's gradient reads may be rewritten once the caller's stream has waited for k, i.e. from the hand-off of
  // component k + 3 on: the derivative matrices those gradients read alternate between two buffers per role (layout_arena).
  const bool lag3 = n->wg_on && n->wg_lag == 3 && n->dC2 != nullptr;
  // Minibatches whose GEMMs fill the chip (no weight-gradient streams): the TRUNK components' statistics start here, where the trunk's forward
  // pass ends -- the caller's stream is about to wait 4.4 ms for the denominator's two latency-bound recursions (xent_behind_den), with the matrix
  // cores and HBM idle; the heads' components follow where all of them used to start, behind the xent head's backward pass.
  const bool early_at_fork = n->early_on && !n->wg_on && !n->early_group && options().ng_early_fork != 0;
  // dropout masks of this minibatch (mask m: tdnn1 = 0, tdnnf layer l = l + 1); null = identity
  const bool drop = n->dropout_masks && n->dropout_proportion > 0.f;
  const float mask_max = drop ? 1.0f + 2.0f * n->dropout_proportion : 1.0f;
  tdnnf_tdnn_indexes ix1;  // one tap at offset 0
  const MatView none{nullptr, 0, 0, 0};
  tdnnf_mat lda_out = M(n->lda_out, N0, lda_dim), pl = M(n->prefinal_l_out, No, S), top;
  tdnnf_mat y = M(n->head[0].y, No, P), dy = M(n->d_y, No, P), dx = M(n->d_xent, No, P), lsm = M(n->xent_logsoftmax, No, P);
  tdnnf_mat d_pl = M(n->d_small, No, S);  // deriv w.r.t. prefinal-l output, summed over both heads
  // ---- state of the step
  bool early_refresh = false;    // a preconditioner refresh was uploaded on s3 (ev_fin recorded): its consumers wait for it
  bool darts_coef_done = false;  // (pl_on: the DARTS components' coefficients and planes were formed at the start of the step)
  std::vector<PlanesSplitArgs> wsplits;  // the weight splits collected for the grouped launch
  unsigned long long coin_k = 0, relu_k = 0;
  // plane operands of this step, by role (empty = the GEMM runs its own kernels)
  std::vector<PlanesOperand> po_in = std::vector<PlanesOperand>(n->layers.size()), po_lin = po_in;
  PlanesOperand po_lda, po_top, po_pl, po_b1[2], po_b2[2], po_dpl;
  // the norm bound of the matrix the next bn_apply_bypass writes (= the next layer's input): from the BatchNorm finalize inside
  // affine_relu_bn_stats; carried to the split at the top of the next layer
  FroBound fb_next;
  PlanesOperand po_next;  // planes of the matrix just written by bn_apply_planes (= the next layer's input), when it wrote them itself
  float *prev = nullptr;  // the trunk's last output so far
  int fused_comp = -1;    // the component whose H_out came with the BatchNorm/ReLU backward sweep; its param_grad call comes next
  bool den_joined = false;   // the caller's stream has waited for the denominator
  bool caller_used = false;  // some component of the open bucket formed its gradient on the caller's stream although wg_on
  float *d_cur = n->dA, *d_next = n->dB;  // d_cur: deriv w.r.t. the current layer's output (noop)

  Step(tdnnf_net *n_, const tdnnf_mat *feats_, const tdnnf_mat *ivectors_, const tdnnf_den_graph *den_, const tdnnf_supervision *sup_, double *results_,
       long long step_, hipStream_t s_, int objective_flags_ = -1)
      : n(n_), feats(feats_), ivectors(ivectors_), den(den_), sup(sup_), results(results_), step(step_), s(s_), objective_flags(objective_flags_) {
    memset(&ix1, 0, sizeof(ix1));
    ix1.row_stride = 1;
    ix1.num_offsets = 1;
  }

  // the reference's RandInt()/RandUniform() coin flips, made reproducible: k-th decision of this minibatch
  int coin() { return (int)(::tdnnf::tdnnf_decision((unsigned long long)step, 2 * coin_k++) & 1); }
  int mark(int k) { return objective ? TDNNF_OK : phase_mark(n, k, s); }  // (an objective call marks no phase boundaries)
  const float *mask_of(int m) const { return drop ? n->dropout_masks + (size_t)m * B * Hd : nullptr; }
  const PlanesOperand *wplanes(int comp) const { return pl_on && n->pw[comp].P ? &n->pw[comp] : nullptr; }
  float *dC_of(int l) const { return !lag3 ? n->dC : (((Ltop - l) & 1) ? n->dC2 : n->dC); }  // d affine-out of tdnnf layer l
  float *dS_of(int l) const { return !lag3 ? nullptr : n->dS[(Ltop - l) & 1]; }              // what layer l's .linear gradient reads
  // stream `to` goes on once everything enqueued on `from` so far is done (one waiter; ev_fork, with up to three, is spelled out)
  static int record_wait(hipEvent_t ev, hipStream_t from, hipStream_t to) {
    TDNNF_HIP(hipEventRecord(ev, from));
    TDNNF_HIP(hipStreamWaitEvent(to, ev, 0));
    return TDNNF_OK;
  }
  // uniform-sample mode runs at most two taps of K (share + sampled)
  bool two_taps(const Tdnn &td) const { return td.darts && (c.darts_flags & TDNNF_DARTS_UNIFORM_SAMPLE) && td.K > 2; }

  // ---- net_step.hip: the schedule
  int run();
  int run_objective();
  int begin();
  int forward_trunk();
  int forward_layer(TdnnfLayer &L, int layer_no);
  int forward_heads_and_objective();
  int forward_head(int h);
  int fork_objective();
  int fork_objective_only();
  int backward_heads();
  int backward_head(int h);
  int backward_trunk();
  int backward_layer(int l);
  int join();
  int capture(const std::string &name, const tdnnf_mat &m);
  double *oderiv_of(double *relu_stats, int relu_index);
  int bn_relu_backward(float *relu_out, const tdnnf_mat &d_in, const tdnnf_mat &d_out, int lead, float *memo, double *relu_stats, float *bias_acc, int comp,
                       int relu_index, const float *mask, FroBound *fb, PlanesOperand *po);
  int affine_relu_bn_stats(int comp, const tdnnf_tdnn_indexes *ix, int K, const PlanesOperand &p_x, const tdnnf_mat *in, const float *eff, tdnnf_mat *out,
                           float *memo, double *stats, FroBound *fb);
  // the untapped affine components (prefinal-l, the heads' .linear and output): y = x W^T [+ bias] and dx = dy W, with the planes of the
  // matrix the GEMM reads (the weights' planes are the component's)
  int affine_forward(int comp, const PlanesOperand &p_x, tdnnf_mat *x, tdnnf_mat *yv);
  int affine_backward_data(int comp, const PlanesOperand &p_dy, tdnnf_mat *dyv, tdnnf_mat *dxv);

  // ---- net_step_planes.hip: plane operands
  tdnnf_net::PlaneSlot *slot_of(const tdnnf_mat &m) const;
  int slot_use(tdnnf_net::PlaneSlot &ps, const tdnnf_mat &m, int lead, long long Rt, int layouts, PlanesOperand *o, bool *same) const;
  int split(const tdnnf_mat &m, int lead, int want, PlanesOperand *o, hipStream_t st, const FroBound &fb = FroBound());
  int next_input_planes(const tdnnf_mat &m, PlanesOperand *o);
  int split_weights(int comp, const float *coef, int period, bool group = false);
  int weight_planes();
  int bwd_planes(const tdnnf_mat &d, int lead, BwdPlanes *bp, PlanesOperand *po);
  int bn_apply_planes(const tdnnf_mat &x, const float *memo, const MatView &byp, float bypass, const tdnnf_mat &out, const float *mask, const FroBound &fb,
                      PlanesOperand *po);
  int transpose_weights();

  // ---- net_step_grad.hip: a component's gradient, the weight-gradient streams, the gradient buckets
  struct WgradSide {
    hipStream_t st;
    void *ws;
    float *scratch;  // split-K scratch (null: the caller's stream with the library's own)
  };
  WgradSide wgrad_side(bool on_caller) const;
  unsigned side_streams() const { return 1u + (n->wg_two ? 1u : 0u) + (n->s5 ? 1u : 0u); }  // weight-gradient streams in use now (<= 3 <= the event ring's lag)
  int wait_last_wgrads(hipStream_t st, unsigned streams);
  int handed_off(hipStream_t sw, bool on_caller);
  int param_grad(int comp, const tdnnf_tdnn_indexes &ix, int K, int Di, int Do, tdnnf_mat *x, tdnnf_mat *dyv, const float *eff, bool bias_done,
                 const int *active, int max_active, bool from_tapgrad);
  int affine_grad(int comp, const PlanesOperand &p_dy, const PlanesOperand &p_x, tdnnf_mat *x, tdnnf_mat *dyv, bool bias_done);
  int tdnn_wgrad(Tdnn &td, const PlanesOperand &p_dy, const PlanesOperand &p_x, tdnnf_mat *x, tdnnf_mat *dyv, const float *eff, bool bias_done);
  float *bias_target(int comp) const;
  int close_bucket(int key);
  // ---- net_step_grad.hip: the natural-gradient scheduling
  std::vector<tdnnf_ng *> all_ng() const;
  int upload_ready_refreshes();
  int finish_refreshes();
  bool is_head_comp(int comp) const;
  bool early_eligible(int comp, int which) const;
  int launch_early_in(int which);
  int out_stats_fuse(int comp, MatView xv, MatView dzv, MatView dv, NgFuse &f);
  int ng_close(int key);
};

}  // namespace tdnnf
