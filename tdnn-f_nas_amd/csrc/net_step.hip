// net_step.hip -- one minibatch of nnet3-chain-train on a tdnnf_net (net.h): tdnnf_net_forward_backward, as a host-side C++
// executor over the component kernels of this library.
//
// Mirrors (UPSTREAM) NnetChainTrainer::TrainInternal:  forward through every component's Propagate,
// chain::ComputeChainObjfAndDeriv, Backprop through every component (raw-gradient / is_gradient_
// UpdateSimple path); the optimizer helpers that follow are tdnnf_net_update (net_update.hip).
//
// The step is one object (Step): its members are the state that lives for one minibatch, its methods the pieces of the schedule,
// and run() lists the phases between the phase_mark boundaries.  State that lives across minibatches stays in tdnnf_net.
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "batchnorm.h"
#include "common.h"
#include "fused.h"
#include "gemm_f32.h"
#include "net_model.h"
#include "ng.h"

namespace tdnnf {
namespace {

// W_acc[o][i*Di + d] += coef[i] * G[o][i*Di + d]   (DARTS: fold the unscaled tap gradients into the accumulator)
__global__ void add_scaled_taps_kernel(const float *G, const float *coef, float *acc, int Do, int KDi, int Di) {
  const long long total = (long long)Do * KDi;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) acc[e] += coef[(e % KDi) / Di] * G[e];
}
// T[o][c] = coef[c / Di] * G[o][c]   (raw gradient of the spliced, coefficient-scaled input from the unscaled tap gradients)
__global__ void scaled_taps_to_kernel(const float *G, const float *coef, int Do, int KDi, int Di, float *T, int ldT) {
  const long long total = (long long)Do * KDi;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int o = (int)(e / KDi), c = (int)(e % KDi);
    T[(size_t)o * ldT + c] = (coef ? coef[c / Di] : 1.0f) * G[e];
  }
}
// ---- bottleneck-dimension supernet (scripts/generate_bottleneckCB8share_onehottrain_config.py:10-85).
struct BnChoice {
  int C, mode;
  int cum[8];  // cumulative block widths: candidate bottleneck dims
  float flops_scale, temp;
};
// p (C): choice probabilities, identical for every row -- mode 0 OnehotFunctionComponent::Propagate
// (nnet-simple-component.cc:9504-9519), 1 SoftmaxFlops :9968-9981 on the ConstantFunction output, 2 GumbelSoftmaxFlops
// :10088-10113 (one noise vector shared by all rows).  mask[c] = sum_{j >= block(c)} p_j: CopyN of Sum(p_k..p_{C-1}).
__global__ void bn_choice_forward_kernel(BnChoice bc, const float *alpha, const float *u, float *p, float *mask) {
  __shared__ float sp[8];
  if (threadIdx.x == 0) {
    const int C = bc.C;
    if (bc.mode == 0) {
      for (int i = 0; i < C; i++) sp[i] = (u[0] >= (float)i / C && u[0] < (float)(i + 1) / C) ? 1.0f : 0.0f;
    } else {
      float v[8], mx = -INFINITY;
      for (int i = 0; i < C; i++) {
        v[i] = bc.mode == 2 ? (alpha[i] + -logf(-logf(u[i]))) * (1.0f / bc.temp) : alpha[i];
        mx = fmaxf(mx, v[i]);
      }
      double sum = 0;
      for (int i = 0; i < C; i++) sum += exp((double)v[i] - mx);
      for (int i = 0; i < C; i++) {
        const float q = (float)(exp((double)v[i] - mx) / sum);
        sp[i] = q < 1.0e-20f ? 1.0e-20f : q;  // ApplyFloor(1e-20)
      }
    }
    for (int i = 0; i < C; i++) p[i] = sp[i];
  }
  __syncthreads();
  const int bn = bc.cum[bc.C - 1];
  for (int c = threadIdx.x; c < bn; c += blockDim.x) {
    int k = 0;
    while (c >= bc.cum[k]) k++;
    float m = 0.f;
    for (int j = k; j < bc.C; j++) m += sp[j];  // Sum(softmax_k, ..., softmax_{C-1}) descriptor
    mask[c] = m;
  }
}
// out[r][c] = in[r][c] * mask[c]   (ElementwiseProductComponent :256-274 / :276-299 with a row-constant factor)
__global__ void col_scale_kernel(MatView in, const float *mask, MatView out) {
  const int C = in.cols;
  const long long total = (long long)in.rows * C;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int r = (int)(e / C), c = (int)(e % C);
    out.data[(size_t)r * out.stride + c] = in.data[(size_t)r * in.stride + c] * mask[c];
  }
}
// Gradient of the C-vector.  partial[chunk][c] = sum over the chunk's rows of lin[r][c] * d_masked[r][c]
// (ElementwiseProduct backprop w.r.t. the CopyN factor), E_j = sum_{c < cum[j]} (CopyN backprop + Sum descriptor).
//   mode 0: grad_j += E_j                                                    (OnehotFunction :9539-9548)
//   mode 1/2: e_j = E_j + flops_scale / C * (-cum[j]);  grad_j += 5 * p_j (e_j - <p, e>) / temp
//             ((Gumbel)SoftmaxFlops backprop summed over rows, then ConstantFunction :2636)
__global__ void bn_choice_backward_kernel(BnChoice bc, const float *partial, int chunks, const float *p, float *grad) {
  __shared__ double dm[512];
  const int bn = bc.cum[bc.C - 1];
  for (int c = threadIdx.x; c < bn; c += blockDim.x) {
    double sacc = 0;
    for (int k = 0; k < chunks; k++) sacc += partial[(size_t)k * bn + c];
    dm[c] = sacc;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double E[8], run = 0;
  int c = 0;
  for (int j = 0; j < bc.C; j++) {
    for (; c < bc.cum[j]; c++) run += dm[c];
    E[j] = run;
  }
  if (bc.mode == 0) {
    for (int j = 0; j < bc.C; j++) grad[j] += (float)E[j];
    return;
  }
  double pe = 0;
  for (int j = 0; j < bc.C; j++) {
    E[j] += (double)bc.flops_scale / bc.C * -(double)bc.cum[j];
    pe += (double)p[j] * E[j];
  }
  for (int j = 0; j < bc.C; j++) grad[j] += 5.0f * (float)(p[j] * (E[j] - pe)) * (1.0f / bc.temp);
}
// partial[chunk][c] = sum_{r in chunk} a[r][c] * b[r][c]
__global__ __launch_bounds__(256) void colsum_prod_partial_kernel(MatView a, MatView b, int rows_per_chunk, float *partial) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  const int r0 = blockIdx.y * rows_per_chunk, r1 = min(a.rows, r0 + rows_per_chunk);
  if (col >= a.cols) return;
  float sacc = 0.f;
  for (int r = r0; r < r1; r++) sacc += a.data[(size_t)r * a.stride + col] * b.data[(size_t)r * b.stride + col];
  partial[(size_t)blockIdx.y * a.cols + col] = sacc;
}
// active[0] = number of taps with a non-zero effective coefficient, active[1..] = their ids
__global__ void active_taps_kernel(const float *eff, int K, int *active) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int n = 0;
  for (int i = 0; i < K; i++)
    if (eff[i] != 0.f) active[1 + n++] = i;
  active[0] = n;
}
// grads += this minibatch's gradient, unless the chain objective failed (results[5] == 0): then, as in the
// reference (derivatives set to zero), the minibatch contributes nothing
__global__ void commit_grads_kernel(float *grads, const float *gtmp, long long n, const double *results) {
  if (results[5] == 0.0) return;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += gridDim.x * 256LL) grads[i] += gtmp[i];
}
// paramsT[begin_c + col * rows + row] = params[begin_c + row * cols + col] for every component c (blockIdx.y)
struct TransTable {
  long long begin[128];
  int rows[128], cols[128];
};
__global__ __launch_bounds__(256) void transpose_weights_kernel(const float *params, float *paramsT, TransTable tb) {
  const int c = blockIdx.y, rows = tb.rows[c], cols = tb.cols[c];
  const float *W = params + tb.begin[c];
  float *WT = paramsT + tb.begin[c];
  const long long total = (long long)rows * cols;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int col = (int)(e / rows), row = (int)(e % rows);  // consecutive threads: consecutive rows of one column -> coalesced writes
    WT[e] = W[(long long)row * cols + col];
  }
}

}  // namespace
}  // namespace tdnnf

using namespace tdnnf;

namespace {

// GeneralDropoutComponent::GetMemo (UPSTREAM), continuous form: mask = 1 - 2p + 4p U, U uniform on (0, 1)
__global__ void dropout_mask_kernel(const float *u, float p, long long n, float *mask) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    mask[i] = 1.0f - 2.0f * p + 4.0f * p * u[i];
}

// BatchNormTestComponent (cv-update): memo rows 0 (mean) and 2 (scale) from the stored statistics, ComputeDerived
// nnet-normalize-component.cc:682-715; rows 3 and 4 (backward terms of the train-mode component) are zero
__global__ void bn_test_memo_kernel(const double *stats, int D, float epsilon, float target_rms, float *memo) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= D) return;
  const double count = stats[0];
  const float off = (float)(stats[1 + d] * (-1.0 / count));
  float sc = (float)(stats[1 + D + d] * (1.0 / count));
  sc += -1.0f * off * off;
  memo[D + d] = sc;
  sc = floor_keep_nan(sc, 0.f) + epsilon;
  sc = target_rms / sqrtf(sc);
  memo[d] = -off;
  memo[2 * D + d] = sc;
  memo[3 * D + d] = 0.f;
  memo[4 * D + d] = 0.f;
}
int bn_test_memo(float *memo, const double *stats, int cols, hipStream_t s) {
  hipLaunchKernelGGL(bn_test_memo_kernel, dim3((cols + 255) / 256), dim3(256), 0, s, stats, cols, 1.0e-3f, 1.0f, memo);
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}
// (store = false, train mode: the statistics block is left as it is -- tdnnf_net_objective without its store flag)
int bn_fwd(tdnnf_net *n, float *in, float *out, int rows, int cols, float *memo, double *stats, hipStream_t s, bool store = true) {
  tdnnf_mat a = M(in, rows, cols), o = M(out, rows, cols);
  if (n->cfg.cv_update) {
    CK(bn_test_memo(memo, stats, cols, s));
    const MatView none{nullptr, 0, 0, 0};
    TDNNF_HIP(bn_apply_bypass(view(&a), memo, cols, ldpad(cols), none, 0.f, view(&o), s));
    return TDNNF_OK;
  }
  CK(tdnnf_batchnorm_propagate(&a, 1.0e-3f, 1.0f, &o, memo, n->ws, n->ws_bytes, s));
  if (!store) return TDNNF_OK;
  return tdnnf_batchnorm_store_stats(memo, cols, rows, stats, s);  // StoreStats runs on every minibatch
}
// Affine (+ bias) + ReLU into `out` and the BatchNorm statistics of that output; the GEMM's epilogue forms the column sums
// while it stores the tile when it can (exact-f32 128-wide tile), otherwise a pass over `out` does.  The normalisation itself
// is applied later by a fused pass.
int affine_relu_bn_stats(tdnnf_net *n, const tdnnf_tdnn_indexes *ix, const tdnnf_mat *in, const float *W, int ldw, int Do, int Di, const float *bias,
                         const float *eff, tdnnf_mat *out, float *memo, double *stats, hipStream_t s, bool store = true) {
  if (n->cfg.cv_update) {
    CK(tdnn_propagate_impl(ix, in, W, ldw, Do, Di, bias, eff, 1, 1, out, s));
    return bn_test_memo(memo, stats, Do, s);
  }
  if (!store) stats = nullptr;  // (bn_fwd)
  int prows = 0;
  const bool room = n->ws_bytes >= sizeof(float) * 2 * (size_t)Do * rows_gemm_colstats_cap(out->rows);
  CK(tdnn_propagate_impl(ix, in, W, ldw, Do, Di, bias, eff, 1, 1, out, s, room ? (float *)n->ws : nullptr, room ? &prows : nullptr));
  // (StoreStats runs on every minibatch: in the finalize launch)
  if (prows > 0) TDNNF_HIP(batchnorm_stats_from_partials((const float *)n->ws, prows, out->rows, Do, 1.0e-3f, 1.0f, memo, s, stats));
  else TDNNF_HIP(batchnorm_stats(view(out), 1.0e-3f, 1.0f, memo, n->ws, s, stats));
  return TDNNF_OK;
}
// statistics of BatchNorm(x) only; the normalisation itself is applied by a fused pass
int bn_stats(tdnnf_net *n, float *x, int rows, int cols, float *memo, double *stats, hipStream_t s) {
  if (n->cfg.cv_update) return bn_test_memo(memo, stats, cols, s);
  tdnnf_mat a = M(x, rows, cols);
  TDNNF_HIP(batchnorm_stats(view(&a), 1.0e-3f, 1.0f, memo, n->ws, s, stats));
  return TDNNF_OK;
}

BnChoice bn_choice(const tdnnf_net_config &c) {
  BnChoice bc;
  memset(&bc, 0, sizeof(bc));
  bc.C = c.bn_num_choices;
  bc.mode = c.bn_mode;
  int run = 0;
  for (int k = 0; k < 8; k++) {
    if (k < bc.C) run += c.bn_choice_dims[k];
    bc.cum[k] = run;
  }
  bc.flops_scale = c.bn_flops_scale;
  bc.temp = c.bn_mode == 2 ? c.bn_temp_proportion : 1.0f;
  return bc;
}

// Few sequences leave most CUs idle while one workgroup per sequence walks the frames: there the backward recursion of the denominator runs beside
// the forward one and the occupancies of all frames at once (the split form).  Measured (ms per step, one-kernel backward -> split): 1500 x 16
// 37.3 -> 28.5, x 32 53.1 -> 45.3, x 64 80.9 -> 75.2, x 128 127.6 -> 128.2; 150 x 64 14.2 -> 13.8.  The second recursion runs on the
// weight-gradient stream (or the natural-gradient side stream), idle until the backward pass (on a stream of its own -- a fifth in flight -- the
// step at 150 x 64 took 20.0 ms: they then share hardware queues).
// [r4] with the pre-split plane GEMMs (planes = true) the xent head no longer covers a 25 ms denominator at 128 sequences: side by side there too
// (same box, ms per step: f16x3 103.8 / 105.2 -> 102.1 / 102.4; exact f32 124.4 / 124.6 -> 125.4 / 125.0, so f32 keeps the one-kernel backward pass)
// [r4, later] with the recursions at 8.8 us per frame (den_persistent_kernels.h, FAST kernels) side by side wins for exact f32 at 128 sequences as well: 122.3 / 122.6 ms
// against 122.7 / 122.9 on one box, and the GEMM launches beside it are stretched less (event-timed 128 x 128 class 0.642 of the peak against 0.617)
bool den_uses_split() { return options().den_split >= 0 ? options().den_split != 0 : true; }

// the first step of a net: the chain workspace and every stream and event of the step, in this order (HIP maps streams to hardware
// queues in creation order)
int create_streams_and_events(tdnnf_net *n, const tdnnf_den_graph *den) {
  n->den_split = den_uses_split();  // latched: option den_split read once per net (the workspace is sized for it)
  n->chain_ws_bytes = tdnnf_chain_workspace_bytes(den, n->B, n->Tout) - (n->den_split ? 0 : chain_split_region_bytes(den, n->B, n->Tout));
  TDNNF_HIP(hipMalloc(&n->chain_ws, n->chain_ws_bytes));
  TDNNF_HIP(hipStreamCreateWithFlags(&n->s2, hipStreamNonBlocking));
  TDNNF_HIP(hipEventCreateWithFlags(&n->ev_fork, hipEventDisableTiming));
  TDNNF_HIP(hipEventCreateWithFlags(&n->ev_den, hipEventDisableTiming));
  TDNNF_HIP(hipEventCreateWithFlags(&n->ev_num, hipEventDisableTiming));
  // The side stream (natural-gradient statistics, the denominator's second recursion) at the default priority, as every stream of the
  // library: rounds 2-3 gave it the lowest priority above 32 sequences, which is worth nothing measurable in the step any more
  // (124.0 / 124.0 ms at 128 sequences, 22.9 / 23.0 at 16) and made a job's step time depend on what had run before it in the
  // process -- once a stream of another priority has existed, HIP's hardware-queue pool maps the next net's streams differently (a
  // 16-sequence step took 35 ms instead of 23 after a 128-sequence job, a 128-sequence step 142 ms after a 16-sequence one;
  // docs/experiments.md r4-d).
  TDNNF_HIP(hipStreamCreateWithFlags(&n->s3, hipStreamNonBlocking));
  TDNNF_HIP(hipEventCreateWithFlags(&n->ev_s3, hipEventDisableTiming));
  TDNNF_HIP(hipEventCreateWithFlags(&n->ev_fin0, hipEventDisableTiming));
  TDNNF_HIP(hipEventCreateWithFlags(&n->ev_fin, hipEventDisableTiming));
  if (n->early_on) {
    TDNNF_HIP(hipEventCreateWithFlags(&n->ev_early_in, hipEventDisableTiming));
    TDNNF_HIP(hipEventCreateWithFlags(&n->ev_early, hipEventDisableTiming));
    n->early.assign(n->comps.size(), tdnnf_net::EarlyIn());
  }
  if (n->early_on && !n->wg_on) TDNNF_HIP(hipStreamCreateWithFlags(&n->s4, hipStreamNonBlocking));
  if (n->wg_on) {
    TDNNF_HIP(hipStreamCreateWithFlags(&n->s4, hipStreamNonBlocking));
    if (n->ws5) TDNNF_HIP(hipStreamCreateWithFlags(&n->s5, hipStreamNonBlocking));
    for (int i = 0; i < 4; i++) TDNNF_HIP(hipEventCreateWithFlags(&n->ev_pg[i], hipEventDisableTiming));
    TDNNF_HIP(hipEventCreateWithFlags(&n->ev_pg_in, hipEventDisableTiming));
  }
  TDNNF_HIP(hipEventCreateWithFlags(&n->ev_ngc, hipEventDisableTiming));
  return TDNNF_OK;
}

// plane operands: split a matrix into its slot and describe it
enum { kP = 1, kT = 2 };
// (optional) norm bound a BatchNorm finalize launch left in n->fro_buf: blocks > 0 -> the split takes its scale from it (planes_gemm.h)
struct FroBound {
  int blocks = 0;
  float mul = 1.0f, add_coef = 0.0f;
  const float *add_rec = nullptr;
};
const PlanesOperand *hint_of(const PlanesOperand &o) { return o.base ? &o : nullptr; }

struct Step {
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
  unsigned side_streams() const { return 1u + (n->wg_two ? 1u : 0u) + (n->s5 ? 1u : 0u); }  // weight-gradient streams in use now (<= 3 <= the event ring's lag)
  std::vector<tdnnf_ng *> all_ng() const {
    std::vector<tdnnf_ng *> v;
    for (auto *list : {&n->ng_in, &n->ng_out})
      for (tdnnf_ng *g : *list)
        if (g) v.push_back(g);
    return v;
  }
  // `st` waits for the last component of each of the `streams` weight-gradient streams in use
  int wait_last_wgrads(hipStream_t st, unsigned streams) {
    for (unsigned b = 1; b <= streams && b <= n->pg_count; b++) TDNNF_HIP(hipStreamWaitEvent(st, n->ev_pg[(n->pg_count - b) & 3], 0));
    return TDNNF_OK;
  }

  // ---------------------------------------------------------------- plane operands
  // whether `ps` last held exactly this split -- (rows, cols, lead, R, layouts): the same again leaves the zero rows as they are -- and the record of it
  static bool slot_same_shape(tdnnf_net::PlaneSlot &ps, const tdnnf_mat &m, int lead, long long R, int layouts) {
    const long long cfg5[5] = {m.rows, m.cols, lead, R, layouts};
    const bool same = memcmp(cfg5, ps.last, sizeof(cfg5)) == 0;
    memcpy(ps.last, cfg5, sizeof(cfg5));
    return same;
  }
  // the slot was allocated (net_arena.hip, by planes_gemm.h's planes_slot_* sizes) for planes of `m` with R rows, and transposed planes with Rt
  // rows (0: none are written): anything larger would be written past its end
  int slot_holds(const tdnnf_net::PlaneSlot &ps, const tdnnf_mat &m, long long R, long long Rt) const {
    TDNNF_REQUIRE(planes_bytes(np, R, planes_slot_kblocks(m.cols)) <= ps.bytesP && planes_bytes(np, Rt, planes_t_kblocks(m.rows)) <= ps.bytesPT,
                  "net_forward_backward: plane slot too small for a %d x %d matrix", m.rows, m.cols);
    return TDNNF_OK;
  }
  // the row-major planes of `m` in slot `ps`, as a GEMM hint
  PlanesOperand slot_operand(const tdnnf_mat &m, const tdnnf_net::PlaneSlot &ps, long long R, int lead, long long kb_alloc) const {
    PlanesOperand o;
    o.base = m.data; o.rows = m.rows; o.cols = m.cols; o.ld = m.stride; o.np = np;
    o.P = ps.P; o.R = R; o.lead = lead; o.kb_alloc = kb_alloc; o.scale = np == 2 ? ps.scale : nullptr;
    return o;
  }
  int split(const tdnnf_mat &m, int lead, int want, PlanesOperand *o, hipStream_t st, const FroBound &fb = FroBound()) {
    *o = PlanesOperand();
    if (!pl_on) return TDNNF_OK;
    auto it = n->plane_slots.find(m.data);
    if (it == n->plane_slots.end() || m.rows <= 0) return TDNNF_OK;  // (no slot: the GEMM runs its own kernels)
    tdnnf_net::PlaneSlot &ps = it->second;
    // a wide matrix (the 1536- / 6034-column activations and derivatives) is the tile-row operand of its weight gradient, which reads
    // the ROW-MAJOR planes through transposing LDS loads: no planes of the transpose for those
    if (m.cols >= 1024) want = kP;
    PlanesSplitArgs a;
    a.np = np; a.x = view(&m); a.scale = ps.scale; a.sumsq_ws = n->planes_ws;
    if (np == 2 && fb.blocks > 0 && (fb.add_coef == 0.f || fb.add_rec)) {
      a.fro2_bound = n->fro_buf; a.fro2_blocks = fb.blocks; a.fro_mul = fb.mul; a.add_coef = fb.add_coef; a.add_rec = fb.add_rec;
    }
    lead = (lead + 15) & ~15;  // (a weight gradient reads the row-major planes in K steps of 16 rows: the matrix starts on one)
    a.lead = lead;
    a.R = planes_slot_rows(m.rows, lead);
    a.Rt = planes_slot_t_rows(m.cols);
    a.P = (want & kP) ? ps.P : nullptr;
    a.PT = (want & kT) ? ps.PT : nullptr;
    const long long kb_alloc = planes_slot_kblocks(m.cols);
    CK(slot_holds(ps, m, a.R, a.Rt));
    a.pads_done = slot_same_shape(ps, m, lead, a.R, want);
    TDNNF_HIP(planes_split(a, st));
    *o = slot_operand(m, ps, a.R, lead, kb_alloc);
    o->P = a.P; o->PT = a.PT; o->Rt = a.Rt;
    return TDNNF_OK;
  }
  // a component's weight matrix as planes (row-major: forward; transposed: backward-data); coef: a TdnnDARTSV3Component's effective tap
  // coefficients (device, one per `period` columns), folded into the planes so that its GEMMs need none
  // (`group`: collect the split instead of launching it -- the plain components' weights of a step go as ONE grouped pair of launches)
  int split_weights(int comp, const float *coef, int period, bool group = false) {
    PlanesOperand &o = n->pw[comp];
    if (!o.P) return TDNNF_OK;
    o.base = net_W(n, comp);
    o.coef = coef;
    o.coef_period = period;
    PlanesSplitArgs a;
    a.np = np; a.x = MatView{net_W(n, comp), o.rows, o.cols, o.cols}; a.lead = 0; a.R = o.R; a.P = const_cast<void *>(o.P); a.Rt = o.Rt;
    a.PT = const_cast<void *>(o.PT); a.scale = n->pw_scale[comp]; a.sumsq_ws = n->planes_ws;
    a.col_coef = coef; a.col_coef_period = period;
    o.scale = np == 2 ? n->pw_scale[comp] : nullptr;
    a.pads_done = n->fb_count > 1;  // (fixed shapes: the zero rows written by the first step stay)
    if (group && options().planes_group && planes_split_group_ok(a)) wsplits.push_back(a);
    else TDNNF_HIP(planes_split(a, s));
    return TDNNF_OK;
  }
  // where the fused BatchNorm / ReLU backward sweep may write the f16 planes of the derivative matrix `d` it produces (f16x3, 1536-wide
  // matrices with a slot): fills *bp for bn_relu_bwd and *po for the GEMMs that read `d` next; bp->P == null: not fused, split afterwards
  int bwd_planes(const tdnnf_mat &d, int lead, BwdPlanes *bp, PlanesOperand *po) {
    *bp = BwdPlanes{nullptr, 0, 0, nullptr};
    *po = PlanesOperand();
    if (!(pl_on && np == 2 && d.cols % 16 == 0 && d.cols >= 1024)) return TDNNF_OK;
    auto it = n->plane_slots.find(d.data);
    if (it == n->plane_slots.end()) return TDNNF_OK;
    tdnnf_net::PlaneSlot &ps = it->second;
    lead = (lead + 15) & ~15;
    const long long R = planes_slot_rows(d.rows, lead), kb_alloc = planes_slot_kblocks(d.cols);
    CK(slot_holds(ps, d, R, 0));
    if (!slot_same_shape(ps, d, lead, R, kP)) TDNNF_HIP(planes_pad(np, ps.P, planes_kblocks(d.cols), R, lead, d.rows, s));
    *bp = BwdPlanes{ps.P, R, lead, ps.scale};
    *po = slot_operand(d, ps, R, lead, kb_alloc);
    return TDNNF_OK;
  }
  // bn_apply_bypass that ALSO writes its output as f16 planes when the BatchNorm finalize left a norm bound (f16x3, plain views): the
  // scale record first (from the bound), then one pass writes the f32 matrix and its row-major planes -- the GEMM that reads `out`
  // next needs no split pass.  *po describes the planes (empty: not fused, the consumer splits).
  int bn_apply_planes(const tdnnf_mat &x, const float *memo, const MatView &byp, float bypass, const tdnnf_mat &out, const float *mask, const FroBound &fb,
                      PlanesOperand *po) {
    *po = PlanesOperand();
    auto it = (pl_on && np == 2 && fb.blocks > 0 && (fb.add_coef == 0.f || fb.add_rec) && out.cols == Hd && out.stride == ldpad(Hd)) ? n->plane_slots.find(out.data)
                                                                                                                                         : n->plane_slots.end();
    if (it == n->plane_slots.end()) {
      TDNNF_HIP(bn_apply_bypass(view(&x), memo, Hd, ldpad(Hd), byp, bypass, view(&out), s, mask, B));
      return TDNNF_OK;
    }
    tdnnf_net::PlaneSlot &ps = it->second;
    const long long R = planes_slot_rows(out.rows, 0), kb_alloc = planes_slot_kblocks(out.cols);
    CK(slot_holds(ps, out, R, 0));
    TDNNF_HIP(planes_scale_bound(n->fro_buf, fb.blocks, (double)out.rows * out.cols, fb.mul, fb.add_coef, fb.add_rec, ps.scale, s));
    const bool held = ps.last[0] >= 0;
    if (!slot_same_shape(ps, out, 0, R, kP) && held) {  // (the slot last held another shape: zero rows behind the matrix again)
      TDNNF_HIP(planes_pad(np, ps.P, planes_kblocks(out.cols), R, 0, out.rows, s));
    }
    const PlanesSink sink{ps.P, R, ps.scale};
    TDNNF_HIP(bn_apply_bypass(view(&x), memo, Hd, ldpad(Hd), byp, bypass, view(&out), s, mask, B, &sink));
    if (options().planes_check_bound) TDNNF_HIP(planes_check_bound(view(&out), ps.scale, n->planes_ws, s));
    *po = slot_operand(out, ps, R, 0, kb_alloc);
    return TDNNF_OK;
  }
  // TdnnDARTSV3Component::Propagate :250-289 for both components of the layer: the tap coefficients and the list of active taps
  int darts_coef(TdnnfLayer &L) {
    for (Tdnn *td : {&L.lin, &L.aff}) {
      const float *u = n->draws + td->draw0;
      CK(tdnnf_tdnn_darts_coef(net_alpha(n, td->comp), td->K, c.darts_flags, c.darts_temp_proportion, u, u + td->K, td->share, td->memo,
                               td->memo + TDNNF_MAX_OFFSETS, s));
      hipLaunchKernelGGL(active_taps_kernel, dim3(1), dim3(64), 0, s, td->memo + TDNNF_MAX_OFFSETS, td->K, td->active);
    }
    return TDNNF_OK;
  }

  // ---------------------------------------------------------------- phases
  int begin() {
    n->fb_count++;
    CK(phase_mark(n, 0, s));
    n->wg_two = false;  // (a step that failed half-way may have left it set)
    TDNNF_HIP(hipMemsetAsync(n->gtmp, 0, sizeof(float) * (size_t)n->num_params, s));
    if (n->ng_bsum_all && n->ng_bsum_floats) TDNNF_HIP(hipMemsetAsync(n->ng_bsum_all, 0, sizeof(float) * n->ng_bsum_floats, s));  // every component's raw bias gradient
    n->pg_count = 0;
    n->early_any = false;
    n->ng_cur.clear();
    // Refreshes whose host part has finished: upload W_{t+1} now, on the side stream, which is idle during the forward pass --
    // otherwise the ~9 small launches of each (18 refreshes per step) sit in front of the component's statistics passes in the
    // backward pass.  Whatever is not ready yet stays with its next use.
    if (!(c.use_natural_gradient && n->s3)) return TDNNF_OK;
    TDNNF_HIP(hipEventRecord(n->ev_fin0, s));
    TDNNF_HIP(hipStreamWaitEvent(n->s3, n->ev_fin0, 0));
    SplitKScratchOverride side_scratch(n->s3_scratch, n->s3_scratch_bytes);
    if (n->ngfin) {  // all of them in five grouped launches, if every host part has finished
      int did = 0;
      CK(ng_fin_run(n->ngfin, n->s3, false, &did));
      early_refresh = did != 0;
    } else {
      for (tdnnf_ng *g : all_ng()) {
        int did = 0;
        CK(ng_finalize_if_ready(g, n->s3, &did));
        early_refresh = early_refresh || did;
      }
    }
    if (early_refresh) TDNNF_HIP(hipEventRecord(n->ev_fin, n->s3));
    return TDNNF_OK;
  }
  // this step's weights as planes (the DARTS components' again in the layer loop, once their coefficients are formed)
  int weight_planes() {
    if (!pl_on) return TDNNF_OK;
    // 36 components x (norm pass + split) were 72 launches of 6 - 12 us, serial on the caller's stream with nothing else in flight: two launches now
    for (size_t i = 0; i < n->comps.size(); i++)
      if (n->comps[i].num_alpha == 0 || n->comps[i].plain) CK(split_weights((int)i, nullptr, 0, true));
    // the TdnnDARTSV3Components' too: their tap coefficients depend on the architecture logits and this step's draws only, so they are formed
    // here, ahead of the layer loop, and the coefficient-folded weight planes join the same two launches
    if (options().planes_group && n->draws) {
      for (auto &L : n->layers) {
        if (!L.lin.darts) continue;
        CK(darts_coef(L));
        CK(split_weights(L.lin.comp, L.lin.memo + TDNNF_MAX_OFFSETS, c.hidden_dim, true));
        CK(split_weights(L.aff.comp, L.aff.memo + TDNNF_MAX_OFFSETS, L.bn, true));
      }
      darts_coef_done = true;
    }
    TDNNF_HIP(planes_split_group(wsplits, &n->wsplit_group, s));
    return TDNNF_OK;
  }
  int transpose_weights() {
    if (n->paramsT) {  // split-bf16 backward-data GEMMs read W^T (k-contiguous B operand)
      TransTable tb;
      memset(&tb, 0, sizeof(tb));
      const int nc = (int)n->comps.size();
      for (int i = 0; i < nc; i++) {
        tb.begin[i] = n->comps[i].begin;
        tb.rows[i] = n->comps[i].rows;
        tb.cols[i] = n->comps[i].cols;
      }
      hipLaunchKernelGGL(transpose_weights_kernel, dim3(256, nc), dim3(256), 0, s, n->params, n->paramsT, tb);
    }
    TDNNF_REQUIRE(n->chain_ws_bytes >= tdnnf_chain_workspace_bytes(den, B, n->Tout) - (n->den_split ? 0 : chain_split_region_bytes(den, B, n->Tout)),
                  "net_forward_backward: denominator graph changed size");
    return TDNNF_OK;
  }

  // ================================================================= forward
  int forward_trunk() {
    tdnnf_mat lda_in = M(n->lda_in, N0, lda_dim);
    CK(tdnnf_splice_input(feats, ivectors, B, 3, &lda_in, s));
    CK(tdnnf_affine_propagate(&lda_in, net_W(n, n->c_lda), lda_dim, net_bias(n, n->c_lda), lda_dim, &lda_out, s));
    tdnnf_mat t1r = M(n->t1_relu, N0, Hd), t1b = M(n->t1_bn, N0, Hd);
    if (drop) {
      TDNNF_REQUIRE(n->draws, "net_forward_backward: dropout needs net_set_random_draws before every step");
      const long long nm = (long long)(c.num_layers + 1) * B * Hd;
      hipLaunchKernelGGL(dropout_mask_kernel, dim3(grid_for(nm, 256)), dim3(256), 0, s, n->draws + n->dropout_draw0, n->dropout_proportion, nm, n->dropout_masks);
    }
    // tdnn1: affine (+bias, ReLU in the GEMM epilogue) -> BatchNorm
    CK(split(lda_out, 0, kP | kT, &po_lda, s));
    {
      PlanesHintScope ph(hint_of(po_lda), wplanes(n->tdnn1.comp));
      FroBoundScope fbs(pl_on ? n->fro_buf : nullptr, &fb_next.blocks);
      CK(affine_relu_bn_stats(n, &ix1, &lda_out, net_W(n, n->tdnn1.comp), lda_dim, Hd, lda_dim, net_bias(n, n->tdnn1.comp), nullptr, &t1r, n->t1_bn_memo,
                              n->t1_bn_stats, s, store_bn));
    }
    fb_next.mul = mask_max;
    CK(bn_apply_planes(t1r, n->t1_bn_memo, none, 0.f, t1b, mask_of(0), fb_next, &po_next));
    prev = n->t1_bn;
    int layer_no = 0;
    for (auto &L : n->layers) CK(forward_layer(L, ++layer_no));
    return mark(1);
  }
  int forward_layer(TdnnfLayer &L, int layer_no) {
    TraceRange trace_layer(("forward tdnnf" + std::to_string(layer_no + 1)).c_str());
    PlanesOperand &p_in = po_in[layer_no - 1], &p_lin = po_lin[layer_no - 1];
    tdnnf_mat in = M(prev, N_of(L.gin, B), Hd);
    tdnnf_mat lin = M(L.lin_out, L.lin.rows_out, L.bn);
    const float *lin_eff = nullptr, *aff_eff = nullptr;
    if (L.lin.darts) {
      TDNNF_REQUIRE(n->draws, "net_forward_backward: a DARTS net needs net_set_random_draws before every step");
      if (!darts_coef_done) CK(darts_coef(L));
      lin_eff = L.lin.memo + TDNNF_MAX_OFFSETS;
      aff_eff = L.aff.memo + TDNNF_MAX_OFFSETS;
      if (pl_on && !darts_coef_done) {  // the effective coefficients folded into this step's weight planes
        CK(split_weights(L.lin.comp, lin_eff, Hd));
        CK(split_weights(L.aff.comp, aff_eff, L.bn));
      }
    }
    // uniform-sample mode runs at most two taps of K (share + sampled): tell the FLOP accounting of the profiler
    ProfFlopsScale taps_active(L.lin.darts && (c.darts_flags & TDNNF_DARTS_UNIFORM_SAMPLE) && L.lin.K > 2 ? 2.0 / L.lin.K : 1.0);
    // (DARTS .linear: bias present but offsets[1] < 0 -> out is zeroed and the bias never added, :237-240)
    if (pl_on) {  // (the planes are also the tile-row operand of this layer's weight gradient)
      if (po_next.base == in.data && po_next.rows == in.rows) p_in = po_next;
      else CK(split(in, 0, kP | kT, &p_in, s, fb_next));
    }
    fb_next = FroBound();
    po_next = PlanesOperand();
    {
      PlanesHintScope ph(hint_of(p_in), wplanes(L.lin.comp));
      CK(tdnnf_tdnn_propagate(&L.lin.ix, &in, net_W(n, L.lin.comp), L.lin.K * Hd, L.bn, Hd, nullptr, lin_eff, 2, &lin, s));
    }
    tdnnf_mat aff_in = lin;
    if (L.c_arch >= 0) {  // bottleneck supernet: column blocks of the linear output times CopyN(Sum(p_k..))
      TDNNF_REQUIRE(n->draws || c.bn_mode == 1, "net_forward_backward: the bottleneck supernet needs net_set_random_draws before every step");
      hipLaunchKernelGGL(bn_choice_forward_kernel, dim3(1), dim3(256), 0, s, bn_choice(c), net_W(n, L.c_arch),
                         n->draws ? n->draws + L.arch_draw0 : nullptr, L.arch_p, L.arch_mask);
      aff_in = M(L.lin_masked, L.lin.rows_out, L.bn);
      hipLaunchKernelGGL(col_scale_kernel, dim3(grid_for((long long)lin.rows * L.bn, 256)), dim3(256), 0, s, view(&lin), L.arch_mask, view(&aff_in));
    }
    if (L.perm) {
      tdnnf_mat src = aff_in;
      aff_in = M(L.lin_perm, L.lin.rows_out, L.bn);
      CK(tdnnf_reorder_rows(&src, B, L.aff.ix.row_stride, 1, &aff_in, s));
    }
    tdnnf_mat relu = M(L.relu_out, L.aff.rows_out, Hd);
    if (pl_on && !L.perm) CK(split(aff_in, 0, kP | kT, &p_lin, s));  // (the linear output, or its masked blocks in the bottleneck supernet)
    {
      PlanesHintScope ph(hint_of(p_lin), wplanes(L.aff.comp));
      FroBoundScope fbs(pl_on ? n->fro_buf : nullptr, &fb_next.blocks);
      CK(affine_relu_bn_stats(n, &L.aff.ix, &aff_in, net_W(n, L.aff.comp), L.aff.K * L.bn, Hd, L.bn, net_bias(n, L.aff.comp), aff_eff, &relu, L.bn_memo, L.bn_stats, s,
                              store_bn));
    }
    // noop = mask * batchnorm(relu) + bypass_scale * (rows of the layer input): its norm bound from the two parts
    fb_next.mul = mask_max;
    fb_next.add_coef = c.bypass_scale;
    fb_next.add_rec = p_in.base ? p_in.scale : nullptr;
    if (c.bypass_scale != 0.f && !fb_next.add_rec) fb_next.blocks = 0;  // (the input was not split: no bound for the sum)
    // noop = Sum(Scale(bypass, input), dropout(batchnorm(relu)))  in one pass
    tdnnf_mat byp = sub_grid_view(prev, L.gin, L.gout, B, Hd);
    tdnnf_mat x = relu, out = M(L.noop_out, L.aff.rows_out, Hd);
    if (byp.rows != out.rows) {  // strided bypass rows: view everything as (n, B*stride) super rows
      x = tdnnf_mat{L.relu_out, L.gout.n, byp.cols, B * ldpad(Hd)};
      out = tdnnf_mat{L.noop_out, L.gout.n, byp.cols, B * ldpad(Hd)};
    }
    if (byp.rows == relu.rows) CK(bn_apply_planes(x, L.bn_memo, view(&byp), c.bypass_scale, out, mask_of(layer_no), fb_next, &po_next));
    else TDNNF_HIP(bn_apply_bypass(view(&x), L.bn_memo, Hd, ldpad(Hd), view(&byp), c.bypass_scale, view(&out), s, mask_of(layer_no), B));
    prev = L.noop_out;
    return TDNNF_OK;
  }

  // ---- natural gradient: pending refreshes, and the input-side statistics that need nothing but forward activations
  int finish_refreshes() {
    if (use_ng && n->ng_grouped) {
      // refreshes still pending when the step began: W_{t+1} of ALL of them now, as grouped launches on the side stream (the host
      // waits for the eigen-decompositions here; the GPU has the forward pass and the denominator in its queues meanwhile)
      if (!n->ngfin) {
        bool ready = false;
        for (tdnnf_ng *g : all_ng()) ready = ready || ng_dim(g) != 0;
        if (ready) CK(ng_fin_create(all_ng(), &n->ngfin));
      }
      if (n->ngfin) {
        int did = 0;
        SplitKScratchOverride side_scratch(n->s3_scratch, n->s3_scratch_bytes);
        CK(ng_fin_run(n->ngfin, n->s3, true, &did));
        if (did) {
          TDNNF_HIP(hipEventRecord(n->ev_fin, n->s3));
          early_refresh = true;
        }
      }
    }
    if (early_refresh) TDNNF_HIP(hipStreamWaitEvent(s, n->ev_fin, 0));  // the preconditioners refreshed on s3 (at the start of the step, or just now)
    return TDNNF_OK;
  }
  bool is_head_comp(int comp) const {
    return comp == n->c_prefinal_l || comp == n->head[0].c_affine || comp == n->head[0].c_linear || comp == n->head[0].c_output ||
           comp == n->head[1].c_affine || comp == n->head[1].c_linear || comp == n->head[1].c_output;
  }
  // input-side statistics of every component whose backward call of the previous minibatch recorded its arguments (and has not come yet
  // in this one) and whose preconditioners exist (the grouped chain will take them): on s4, behind the forward pass and the refresh uploads
  bool early_eligible(int comp, int which) const {
    const auto &E = n->early[comp];
    if (E.done == n->fb_count || (which == 0 && is_head_comp(comp))) return false;
    if (E.recorded != n->fb_count - 1 || !n->ng_in[comp] || !n->ng_out[comp] || ng_dim(n->ng_in[comp]) == 0 || ng_dim(n->ng_out[comp]) == 0) return false;
    return n->comps[comp].lr_factor != 0.f && n->ngc[comp].H_in;
  }
  // which: 0 the trunk's components (their inputs exist once the trunk's forward pass is enqueued), 1 the heads' (and whatever was not launched yet), 2 all
  int launch_early_in(int which) {
    if (!(use_ng && n->early_on)) return TDNNF_OK;
    std::vector<int> who;
    for (int comp = (int)n->comps.size() - 1; comp >= 0; comp--)
      if (early_eligible(comp, which)) who.push_back(comp);
    if (who.empty()) return TDNNF_OK;
    TDNNF_HIP(hipEventRecord(n->ev_early_in, s));
    TDNNF_HIP(hipStreamWaitEvent(n->s4, n->ev_early_in, 0));
    if (early_refresh) TDNNF_HIP(hipStreamWaitEvent(n->s4, n->ev_fin, 0));
    NgInput xin;
    if (n->early_group) {  // one grouped launch on s4 (behind the numerator, in front of the heads' weight gradients; s3 carries the denominator's second recursion)
      std::vector<RowsGemmArgs> calls;
      std::vector<int> grouped;
      for (int comp : who) {
        memcpy(&xin, n->early[comp].xin, sizeof(xin));
        RowsGemmArgs a;
        CK(ng_stats_main_prepare(n->ng_in[comp], xin, n->ngc[comp].H_in, n->ngc[comp].part_in, n->s4, &a));
        if (!rows_gemm_group_ok(a)) continue;  // (this one in its own gradient call, as without the early launch)
        calls.push_back(a);
        grouped.push_back(comp);
      }
      if (calls.empty()) return TDNNF_OK;
      TDNNF_HIP(rows_gemm_group(calls, &n->early_launch, n->s4));
      for (int comp : grouped) n->early[comp].done = n->fb_count;
    } else {
      SplitKScratchOverride early_scratch(n->s4_scratch, n->s4_scratch_bytes);
      for (int comp : who) {
        memcpy(&xin, n->early[comp].xin, sizeof(xin));
        CK(ng_stats_main(n->ng_in[comp], xin, n->ngc[comp].H_in, n->ngc[comp].part_in, n->ws4, n->ws_bytes, n->s4));
        n->early[comp].done = n->fb_count;
      }
    }
    TDNNF_HIP(hipEventRecord(n->ev_early, n->s4));
    n->early_any = true;
    return TDNNF_OK;
  }

  int forward_heads_and_objective() {
    if (early_at_fork && !objective) {
      CK(finish_refreshes());
      CK(launch_early_in(0));
    }
    top = M(prev, No, Hd);
    if (po_next.base == top.data && po_next.rows == top.rows) po_top = po_next;
    else CK(split(top, 0, kP | kT, &po_top, s, fb_next));
    {
      PlanesHintScope ph(hint_of(po_top), wplanes(n->c_prefinal_l));
      CK(tdnnf_affine_propagate(&top, net_W(n, n->c_prefinal_l), Hd, nullptr, S, &pl, s));
    }
    CK(split(pl, 0, kP | kT, &po_pl, s));
    for (int h = 0; h < 2; h++) {
      CK(forward_head(h));
      if (h == 0) CK(objective ? fork_objective_only() : fork_objective());
    }
    tdnnf_mat yx = M(n->head[1].y, No, P);
    if (objective) {  // no derivative: the plain LogSoftmax, the xent objective from the posterior pass, then the join of both side streams
      CK(tdnnf_log_softmax_propagate(&yx, &lsm, s));
      TDNNF_HIP(hipStreamWaitEvent(s, n->ev_num, 0));
      CK(chain_objf_num_xent(den, sup, &y, &lsm, n->chain_ws, s));
      TDNNF_HIP(hipStreamWaitEvent(s, n->ev_den, 0));
      return chain_objf_finish(den, sup, &y, c.chain_l2_regularize, results, n->chain_ws, s);
    }
    // xent head: LogSoftmax, numerator posteriors, LogSoftmax backward.  The derivative handed to LogSoftmax is xent_regularize *
    // weight * (posteriors of a frame: they sum to 1), so its backward pass is -xent_regularize * weight * softmax -- written by the
    // forward kernel while the row is in registers -- plus the posteriors the numerator kernel adds on top.
    const bool dense_first = log_softmax_propagate_with_aux(&yx, &lsm, &dx, -c.xent_regularize * chain_supervision_weight(sup), s);
    if (!dense_first) CK(tdnnf_log_softmax_propagate(&yx, &lsm, s));
    // objective, part 2: numerator recursion -> xent_deriv (+)= xent_regularize * posteriors, xent objective
    TDNNF_HIP(hipStreamWaitEvent(s, n->ev_num, 0));
    CK(chain_num_xent(den, sup, &y, &lsm, c.xent_regularize, &dx, n->chain_ws, s, dense_first));
    if (!dense_first) CK(tdnnf_log_softmax_backprop(&lsm, &dx, &dx, s));  // in place into d_xent
    return mark(2);
  }
  int forward_head(int h) {
    auto &H = n->head[h];
    tdnnf_mat ar = M(H.aff_relu, No, Hd), lo = M(H.lin_out, No, S), b1 = M(H.bn1_out, No, Hd), b2 = M(H.bn2_out, No, S), yh = M(H.y, No, P);
    FroBound fb_b1;
    {
      PlanesHintScope ph(hint_of(po_pl), wplanes(H.c_affine));
      FroBoundScope fbs(pl_on ? n->fro_buf : nullptr, &fb_b1.blocks);
      CK(affine_relu_bn_stats(n, &ix1, &pl, net_W(n, H.c_affine), S, Hd, S, net_bias(n, H.c_affine), nullptr, &ar, H.bn1_memo, H.bn1_stats, s, store_bn));
    }
    CK(bn_apply_planes(ar, H.bn1_memo, none, 0.f, b1, nullptr, fb_b1, &po_b1[h]));
    if (!po_b1[h].base) CK(split(b1, 0, kP | kT, &po_b1[h], s, fb_b1));
    {
      PlanesHintScope ph(hint_of(po_b1[h]), wplanes(H.c_linear));
      CK(tdnnf_affine_propagate(&b1, net_W(n, H.c_linear), Hd, nullptr, S, &lo, s));
    }
    CK(bn_fwd(n, H.lin_out, H.bn2_out, No, S, H.bn2_memo, H.bn2_stats, s, store_bn));
    CK(split(b2, 0, kP | kT, &po_b2[h], s));
    PlanesHintScope ph(hint_of(po_b2[h]), wplanes(H.c_output));
    return tdnnf_affine_propagate(&b2, net_W(n, H.c_output), S, net_bias(n, H.c_output), P, &yh, s);
  }
  // ====================================================== objective, part 1 (second stream)
  // The denominator forward-backward (one workgroup per sequence) only needs the chain head's output: it
  // runs on n->s2 while this stream does the xent head forward, the numerator and the xent head backward.
  int fork_objective() {
    TraceRange trace_den("chain denominator forward-backward (second stream)");
    TDNNF_HIP(hipEventRecord(n->ev_fork, s));
    TDNNF_HIP(hipStreamWaitEvent(n->s2, n->ev_fork, 0));
    // few sequences leave most CUs idle while one workgroup per sequence walks the frames: there the backward recursion runs
    // beside the forward one (den_beta_kernel on a further stream) and the occupancies of all frames at once
    const bool den_split = n->den_split;
    TDNNF_HIP(hipStreamWaitEvent(n->s3, n->ev_fork, 0));
    // (option xent_behind_den: the xent head's forward GEMMs start when the recursions are done.  Beside the recursions' 1024-thread workgroups,
    // which hold half the CUs for 4.4 ms, those GEMMs run at 94 instead of 103 TFLOP/s exact f32 (157 instead of 183 f32-equivalent on the plane
    // kernels) -- and the step takes as long either way: three interleaved pairs 120.15 / 120.32 ms exact f32, 82.66 / 82.72 f16x3.  Rounds 2-4
    // had this order by accident, through a 1024-thread BatchNorm finalize block that could not start beside the recursions.  Kept explicit:
    // the same step, GEMM launches that are not stretched by a neighbour.)
    const int xbd = options().xent_behind_den;
    const bool behind = den_split && (xbd > 0 || (xbd < 0 && !n->wg_on));
    if (behind && !n->ev_den_rec) TDNNF_HIP(hipEventCreateWithFlags(&n->ev_den_rec, hipEventDisableTiming));
    bool rec = false;
    CK(chain_den(den, sup, &y, c.leaky_hmm, &dy, n->chain_ws, n->s2, !den_split, n->s3, behind ? n->ev_den_rec : nullptr, &rec));
    if (rec) TDNNF_HIP(hipStreamWaitEvent(s, n->ev_den_rec, 0));
    TDNNF_HIP(hipEventRecord(n->ev_den, n->s2));
    // ... and so does the numerator's forward-backward recursion (one wave per sequence): on a stream that is idle until the
    // backward pass -- the weight-gradient stream when there is one, else behind the second recursion on the side stream
    hipStream_t sn = n->s3;
    if (n->wg_on && den_split) {
      sn = n->s4;
      TDNNF_HIP(hipStreamWaitEvent(sn, n->ev_fork, 0));
    }
    CK(chain_num_recursion(sup, den, &y, n->chain_ws, sn));
    TDNNF_HIP(hipEventRecord(n->ev_num, sn));
    return TDNNF_OK;
  }

  // tdnnf_net_objective: the denominator's forward recursion alone on n->s2, the numerator's recursion on n->s3 (both idle in such a call),
  // beside the xent head's forward pass; forward_heads_and_objective joins both
  int fork_objective_only() {
    TraceRange trace_den("chain denominator forward (second stream)");
    TDNNF_HIP(hipEventRecord(n->ev_fork, s));
    TDNNF_HIP(hipStreamWaitEvent(n->s2, n->ev_fork, 0));
    TDNNF_HIP(hipStreamWaitEvent(n->s3, n->ev_fork, 0));
    CK(chain_objf_den(den, sup, &y, c.leaky_hmm, n->chain_ws, n->s2));
    TDNNF_HIP(hipEventRecord(n->ev_den, n->s2));
    CK(chain_objf_num_recursion(sup, den, &y, n->chain_ws, n->s3));
    TDNNF_HIP(hipEventRecord(n->ev_num, n->s3));
    return TDNNF_OK;
  }

  // ================================================================= backward
  // parity aid: keep a copy of a derivative matrix under `name` (tdnnf_net_set_capture); the originals are recycled scratch
  int capture(const std::string &name, const tdnnf_mat &m) {
    if (!n->capture_on) return TDNNF_OK;
    tdnnf_mat *dst = nullptr;
    for (auto &kv : n->named)
      if (kv.first == name) dst = &kv.second;
    if (!dst) {
      float *p = nullptr;
      TDNNF_HIP(hipMalloc((void **)&p, sizeof(float) * (size_t)std::max(1, m.rows) * ldpad(m.cols)));
      n->captured.push_back(p);
      n->named.push_back({name, M(p, m.rows, m.cols)});
      dst = &n->named.back().second;
    }
    TDNNF_REQUIRE(dst->rows == m.rows && dst->cols == m.cols, "net_forward_backward: captured %s changed shape", name.c_str());
    return tdnnf_sum_scaled(&m, 1.0f, nullptr, 0.f, dst, s);
  }
  int out_stats_fuse(int comp, MatView xv, MatView dzv, MatView dv, NgFuse &f) {  // 1: f is to be passed on
    fused_comp = -1;
    if (!c.use_natural_gradient || n->ng_out.empty() || !n->ng_out[comp] || n->comps[comp].lr_factor == 0.f) return 0;
    if (options().ng_fuse == 0) return 0;  // the statistic by its own GEMM
    const bool fuse_always = options().ng_fuse == 2;  // fused whatever the row count
    auto &C = n->ngc[comp];
    const float *W = nullptr;
    int Rp = 0, ldw = 0;
    CK(ng_external_begin(n->ng_out[comp], dv.cols, &W, &Rp, &ldw, s));
    if (!W || !bn_relu_bwd_ng_ok(xv, dzv, dv, Rp) || !(fuse_always || bn_relu_bwd_ng_pays(dv.rows))) return 0;
    f.W = W; f.Rp = Rp; f.ldw = ldw; f.H = C.H_out; f.part = C.part_out; f.part_cap = rows_gemm_sumsq_blocks(dv.rows);
    fused_comp = comp;
    return 1;
  }
  // NonlinearComponent::StoreBackpropStats (nnet-component-itf.cc:461-480): "if (RandInt(0, 3) == 0 && oderiv_count_ != 0) return"
  // -- three minibatches in four, always the first; a decision stream of its own (the k-th ReLU of the backward pass)
  double *oderiv_of(double *relu_stats, int relu_index) {  // relu_index: the k-th ReLU of stat_blocks() (net_model.h); every ReLU is Hd wide
    std::vector<char> &nz = *n->oderiv_nonzero;
    if ((int)nz.size() < c.num_layers + 3) nz.resize(c.num_layers + 3, 0);
    const bool skip = nz[relu_index] && ::tdnnf::tdnnf_decision((unsigned long long)step, 2 * (4096 + relu_k)) % 4 == 0;
    relu_k++;
    if (!skip) nz[relu_index] = 1;
    return skip ? nullptr : relu_stats + relu_oderiv_at(Hd);
  }
  // BatchNorm backward + ReLU backward (+ StoreStats / self-repair coin flips as in the reference:
  // RectifiedLinearComponent::StoreStats nnet-simple-component.cc:1084, RepairGradients :1017) in two fused
  // passes; also yields the bias gradient of the affine layer in front of the ReLU.
  // With natural gradient the same sweep also forms the output-side statistic H = dY Wy^T of the affine component in front
  // of the ReLU (fused.h NgFuse): into the buffer set the component's param_grad call, which must come next, will take.
  // d_in -> d_out (the same matrix: in place).  *fb: the norm bound the sweep's finalize launch leaves for a split of d_out.  *po
  // receives the plane operand of d_out (`lead` zero rows in front) when the sweep wrote its f16 planes itself (bwd_planes), else
  // stays as it is and the caller splits.  (The FroBoundScope opens behind out_stats_fuse, which starts no BatchNorm finalize; it holds a
  // buffer exactly when pl_on, which bwd_planes asks for itself.)
  int bn_relu_backward(float *relu_out, const tdnnf_mat &d_in, const tdnnf_mat &d_out, int lead, float *memo, double *relu_stats, float *bias_acc, int comp,
                       int relu_index, const float *mask, FroBound *fb, PlanesOperand *po) {
    const bool store = coin() || step == 0;
    const bool repair = c.relu_self_repair_scale > 0.f && coin();
    tdnnf_mat x = M(relu_out, d_in.rows, Hd);
    NgFuse f;
    const int fuse = out_stats_fuse(comp, view(&x), view(&d_in), view(&d_out), f);
    if (fuse < 0) return TDNNF_EINVAL;
    FroBoundScope fbs(pl_on ? n->fro_buf : nullptr, &fb->blocks);
    BwdPlanes bp{nullptr, 0, 0, nullptr};
    PlanesOperand tmp;
    CK(bwd_planes(d_out, lead, &bp, &tmp));
    TDNNF_HIP(bn_relu_bwd(view(&x), view(&d_in), memo, 1.0f, cv, relu_stats, store, repair, c.relu_self_repair_scale, view(&d_out), bias_acc, 1.0f,
                          n->ws, n->ws_bytes, s, mask, B, fuse ? &f : nullptr, oderiv_of(relu_stats, relu_index), bp.P ? &bp : nullptr));
    if (bp.P) *po = tmp;
    if (bp.P && options().planes_check_bound) TDNNF_HIP(planes_check_bound(view(&d_out), bp.rec, n->planes_ws, s));
    return TDNNF_OK;
  }
  // A bucket of the flat gradient buffer is final once the last of its components (in backward order) has been enqueued:
  // grads[range] += this minibatch's gradient (unless the objective failed), then the bucket's event.  With natural gradient
  // the components' commits run on the side stream, so the bucket's commit follows them there.
  int close_bucket(int key) {
    if (use_ng) CK(ng_close(key));
    for (auto &gb : n->buckets) {
      if (gb.close_key != key) continue;
      hipStream_t cs = s;
      if (!use_ng && n->wg_on && n->pg_count > 0) CK(wait_last_wgrads(s, side_streams()));  // the components' gradients were formed on s4 (and s2)
      if (use_ng) {
        TDNNF_HIP(hipEventRecord(gb.handoff, s));  // s-side writes of the range (bias sums, architecture parameters) are done
        TDNNF_HIP(hipStreamWaitEvent(n->s3, gb.handoff, 0));
        cs = n->s3;
      }
      const long long cnt = gb.end - gb.begin;
      if (cnt > 0)
        hipLaunchKernelGGL(commit_grads_kernel, dim3(grid_for(cnt, 256)), dim3(256), 0, cs, n->grads + gb.begin, n->gtmp + gb.begin, cnt, results);
      TDNNF_HIP(hipEventRecord(gb.ready, cs));
    }
    return TDNNF_OK;
  }
  float *bias_target(int comp) const {  // where a fused backward pass should accumulate the raw bias gradient
    if (n->comps[comp].lr_factor == 0.f) return nullptr;  // "if (to_update && learning_rate != 0)": no model derivative
    if (!use_ng) return net_Bg(n, comp);
    return n->ngc[comp].bsum;  // (zeroed with all the others at the start of the step)
  }
  // after this component is enqueued (on sw) the caller's stream may only run ahead of it, not of the one before: what that one reads
  // (derivative scratch, the bias sums) is rewritten from here on
  int handed_off(hipStream_t sw, bool on_caller) {
    if (!n->wg_on || on_caller) return TDNNF_OK;
    // (a ring of four events; wg_lag 1: the caller's stream waits for the component before this one, 3: for the one three back --
    // every component is waited for exactly once either way, so "waited for k" means every component up to k has finished)
    TDNNF_HIP(hipEventRecord(n->ev_pg[n->pg_count & 3], sw));
    const unsigned lag = lag3 ? 3u : 1u;
    if (n->pg_count >= lag) TDNNF_HIP(hipStreamWaitEvent(s, n->ev_pg[(n->pg_count - lag) & 3], 0));
    n->pg_count++;
    return TDNNF_OK;
  }
  // Gradient of one component's weights [+ bias] from its input (tap views) and output derivative.
  //   raw:  W += c_i dY^T X_i, bias += colsum(dY)                      (UpdateSimple, :433-455)
  //   NG :  X~ = [c_i X_i ..., 1], (X~', a) = NG_in(X~), (dY', b) = NG_out(dY), W += a b dY'^T X~'[:, :K Di],
  //         bias += a b dY'^T X~'[:, -1]                               (UpdateNaturalGradient, :592-624)
  //         computed as a b (I - Wy^T Wy) [raw gradient] (I - Wx^T Wx): see ng.h.
  // bias_done: the raw bias gradient was already produced by the fused BatchNorm/ReLU backward pass (into Bg(), or
  // into n->ngBias when natural gradient is on).  tapgrad: unscaled per-tap gradients already in n->tapgrad.
  int param_grad(int comp, const tdnnf_tdnn_indexes &ix, int K, int Di, int Do, tdnnf_mat *x, tdnnf_mat *dyv, const float *eff, bool bias_done,
                 const int *active, int max_active, bool from_tapgrad) {
    const int ldw = K * Di;
    float *bias_acc = net_Bg(n, comp);
    if (n->comps[comp].lr_factor == 0.f) return TDNNF_OK;  // frozen component (cv-update): the reference skips its update
    // sw: where the gradient is formed -- the weight-gradient stream (its inputs are final on s now), or s itself
    hipStream_t sw = s;
    void *wsw = n->ws;
    // Small minibatches: the weight-gradient side (gradient GEMM + slab reduce + the natural-gradient passes of the component) is the longer
    // chain of the two -- 216 us per component against 145 on the caller's stream at 150 x 64 -- and the caller may only run one component
    // ahead of it.  From the denominator's join on its stream is idle: components alternate between the two (event parity = stream parity).
    // (option wgrad_on_caller: the xent head's components -- before the denominator's join, with the input-side statistics of the whole net
    // queued on s4 in front of them -- form their gradients on the caller's stream, which waits for the denominator anyway)
    const bool on_caller = n->wg_on && options().wgrad_on_caller != 0 && n->early_any && !den_joined;
    if (on_caller) caller_used = true;
    // which of the weight-gradient streams: s4 [s5] before the denominator's join, s4 s2 [s5] in turn after it
    float *scr = nullptr;
    if (n->wg_on && !on_caller) {
      const int ns = (n->wg_two ? 2 : 1) + (n->s5 ? 1 : 0), k = (int)(n->pg_count % (unsigned)ns);
      const int which = k == 0 ? 0 : (k == 1 && n->wg_two) ? 1 : 2;  // 0: s4, 1: s2, 2: s5
      sw = which == 0 ? n->s4 : which == 1 ? n->s2 : n->s5;
      wsw = which == 0 ? n->ws4 : which == 1 ? n->ws2 : n->ws5;
      scr = which == 0 ? n->s4_scratch : which == 1 ? n->s2_scratch : n->s5_scratch;
      TDNNF_HIP(hipEventRecord(n->ev_pg_in, s));
      TDNNF_HIP(hipStreamWaitEvent(sw, n->ev_pg_in, 0));
    }
    SplitKScratchOverride sw_scratch(scr, scr ? n->s4_scratch_bytes : 0);
    if (!use_ng) {
      CK(tdnn_update_simple_impl(&ix, x, dyv, Do, Di, eff, 1.0f, net_Wg(n, comp), ldw, bias_done ? nullptr : bias_acc, wsw, n->ws_bytes, active, max_active, sw));
      return handed_off(sw, on_caller);
    }
    const int N = dyv->rows, ones = bias_acc ? 1 : 0, Dx = ldw + ones, ldT = (Dx + 3) & ~3;
    auto &C = n->ngc[comp];
    TDNNF_REQUIRE(C.T && C.N == N, "net_forward_backward: component %s has no natural-gradient buffers for %d rows", n->comps[comp].name.c_str(), N);
    float *T = C.T;
    // grouped chain: once both preconditioners exist (from the second minibatch on)
    const bool grouped = n->ng_grouped && ng_dim(n->ng_in[comp]) != 0 && ng_dim(n->ng_out[comp]) != 0;
    // the gradient GEMM writes T[:, :K Di] itself when it computes every tap; the bias column and the row padding come with
    // ng_set_column (the group's first launch) -- no zero fill of the 2-20 MB block first.  (With tap coefficients a zero one
    // makes the reduce kernel skip its columns: those launches start from zeros.)
    const bool overwrite = !from_tapgrad && !active && eff == nullptr && (ones || ldT == ldw);
    if (!overwrite) TDNNF_HIP(hipMemsetAsync(T, 0, sizeof(float) * (size_t)Do * ldT, sw));
    if (from_tapgrad)
      hipLaunchKernelGGL(scaled_taps_to_kernel, dim3(grid_for((long long)Do * ldw, 256)), dim3(256), 0, sw, n->tapgrad, eff, Do, ldw, Di, T, ldT);
    else
      CK(tdnn_update_simple_impl(&ix, x, dyv, Do, Di, eff, 1.0f, T, ldT, nullptr, wsw, n->ws_bytes, active, max_active, sw, overwrite));
    if (ones) {
      if (!bias_done) TDNNF_HIP(colsum_add(view(dyv), 1.0f, C.bsum, wsw, sw));  // (otherwise the fused ReLU backward pass on s filled it)
      if (!grouped) ng_set_column(C.bsum, Do, T, ldT, ldw, sw);
    }
    // ---- the passes over the N-sized operands
    NgInput xin;
    memset(&xin, 0, sizeof(xin));
    xin.x = view(x); xin.ix = ix; xin.Di = Di; xin.ones = ones; xin.N = N; xin.eff = eff; xin.active = active; xin.max_active = max_active;
    static_assert(sizeof(NgInput) <= sizeof(tdnnf_net::EarlyIn::xin), "EarlyIn::xin too small");
    if (n->early_on && n->early[comp].done == n->fb_count) {
      // H_in (and J on a refresh) were formed ahead of the backward pass from the arguments recorded one minibatch ago: they must be these
      TDNNF_REQUIRE(memcmp(n->early[comp].xin, &xin, sizeof(xin)) == 0, "net_forward_backward: the input of component %s moved between minibatches",
                    n->comps[comp].name.c_str());
      if (n->early_group) {  // H came with the grouped launch on s3: the bookkeeping -- and J of a refresh step -- here, behind it
        TDNNF_HIP(hipStreamWaitEvent(sw, n->ev_early, 0));
        CK(ng_stats_main_finish(n->ng_in[comp], xin, C.H_in, wsw, n->ws_bytes, sw));
      }
    } else {
      CK(ng_stats_main(n->ng_in[comp], xin, C.H_in, C.part_in, wsw, n->ws_bytes, sw));
    }
    if (n->early_on) {
      memcpy(n->early[comp].xin, &xin, sizeof(xin));
      n->early[comp].recorded = n->fb_count;
    }
    NgInput yin;
    memset(&yin, 0, sizeof(yin));
    yin.x = view(dyv); yin.ix.row_stride = 1; yin.ix.num_offsets = 1; yin.Di = Do; yin.N = N;
    if (fused_comp == comp) {  // H_out and its partials came with the BatchNorm/ReLU backward sweep
      fused_comp = -1;
      CK(ng_stats_main_finish(n->ng_out[comp], yin, C.H_out, wsw, n->ws_bytes, sw));
    } else {
      CK(ng_stats_main(n->ng_out[comp], yin, C.H_out, C.part_out, wsw, n->ws_bytes, sw));
    }
    if (grouped) {  // the rest comes with the bucket (ng_close)
      n->ng_cur.push_back(comp);
      CK(handed_off(sw, on_caller));
      if (from_tapgrad && n->wg_on) TDNNF_HIP(hipStreamWaitEvent(s, n->ev_pg[(n->pg_count - 1) & 3], 0));
      return TDNNF_OK;
    }
    // ---- per-object chain (first minibatch): the R x R work, the projections of the raw gradient and the commit, on the side stream
    TDNNF_HIP(hipEventRecord(n->ev_ngc, sw));
    TDNNF_HIP(hipStreamWaitEvent(n->s3, n->ev_ngc, 0));
    {
      SplitKScratchOverride side_scratch(n->s3_scratch, n->s3_scratch_bytes);
      CK(ng_chain_one(n->ng_in[comp], n->ng_out[comp], C.H_in, C.part_in, C.H_out, C.part_out, T, Do, Dx, ldT, ldw, net_Wg(n, comp), bias_acc,
                      n->ng_side_ws, n->ngset_ws_bytes, n->ngTmp, n->s3));
    }
    CK(handed_off(sw, on_caller));
    // (the unscaled tap gradients this one reads are rebuilt by the next DARTS component on the caller's stream)
    if (from_tapgrad && n->wg_on) TDNNF_HIP(hipStreamWaitEvent(s, n->ev_pg[(n->pg_count - 1) & 3], 0));
    return TDNNF_OK;
  }
  // Natural gradient, grouped: the chains of the components enqueued since the last bucket closed, as one sequence of grouped
  // launches on the side stream behind their N-sized passes.
  int ng_close(int key) {
    if (n->ng_cur.empty()) return TDNNF_OK;
    bool closes = false;  // (called after every layer: only those that end a gradient bucket run the chain)
    for (auto &gb : n->buckets) closes = closes || gb.close_key == key;
    if (!closes) return TDNNF_OK;
    tdnnf_net::NgBucket *nb = nullptr;
    for (auto &b : n->ng_buckets)
      if (b.key == key) nb = &b;
    if (!nb) {
      std::vector<NgGroupComp> gc;
      for (int comp : n->ng_cur) {
        const CompDesc &cd = n->comps[comp];
        auto &C = n->ngc[comp];
        NgGroupComp g;
        g.in = n->ng_in[comp]; g.out = n->ng_out[comp];
        g.T = C.T; g.Do = cd.rows; g.ldw = cd.cols; g.Dx = cd.cols + (cd.has_bias ? 1 : 0); g.ldT = (g.Dx + 3) & ~3;
        g.bsum = cd.has_bias ? C.bsum : nullptr;
        g.H_in = C.H_in; g.H_out = C.H_out; g.part_in = C.part_in; g.part_out = C.part_out; g.N = C.N;
        g.W_acc = net_Wg(n, comp); g.bias_acc = net_Bg(n, comp);
        gc.push_back(g);
      }
      NgGroup *grp = nullptr;
      CK(ng_group_create(gc, &grp));
      n->ng_buckets.push_back(tdnnf_net::NgBucket{key, n->ng_cur, grp});
      nb = &n->ng_buckets.back();
    }
    TDNNF_REQUIRE(nb->comps == n->ng_cur, "net_forward_backward: the components of gradient bucket %d changed between minibatches", key);
    // behind the last component's passes (on the weight-gradient stream when that is on)
    if (n->wg_on && n->pg_count > 0) {
      CK(wait_last_wgrads(n->s3, side_streams()));
      if (caller_used) {
        TDNNF_HIP(hipEventRecord(n->ev_ngc, s));
        TDNNF_HIP(hipStreamWaitEvent(n->s3, n->ev_ngc, 0));
        caller_used = false;
      }
    } else {
      TDNNF_HIP(hipEventRecord(n->ev_ngc, s));
      TDNNF_HIP(hipStreamWaitEvent(n->s3, n->ev_ngc, 0));
    }
    if (n->early_any) TDNNF_HIP(hipStreamWaitEvent(n->s3, n->ev_early, 0));  // the H_in of this step (all of them: one event)
    CK(ng_group_run(nb->group, n->s3));
    n->ng_cur.clear();
    return TDNNF_OK;
  }
  // weight gradient of one Tdnn component.  DARTS in a non-sampling mode also needs the architecture-logit
  // gradient (UpdateNaturalGradient :516-590): tap gradients are formed unscaled once, s_i = <dW_i, W_i>
  // replaces the reference's extra forward GEMM per tap, then c_i * dW_i goes into the accumulator.
  int tdnn_wgrad(Tdnn &td, tdnnf_mat *x, tdnnf_mat *dyv, const float *eff, bool bias_done) {
    const int ldw = td.K * td.Di;
    bool tap_ready = false;
    if (td.darts && !(c.darts_flags & TDNNF_DARTS_UNIFORM_SAMPLE)) {
      tap_ready = true;
      TDNNF_HIP(hipMemsetAsync(n->tapgrad, 0, sizeof(float) * (size_t)td.Do * ldw, s));
      CK(tdnnf_tdnn_update_simple(&td.ix, x, dyv, td.Do, td.Di, nullptr, 1.0f, n->tapgrad, ldw, nullptr, n->ws, n->ws_bytes, s));
      CK(tdnnf_tdnn_darts_alpha_update(n->tapgrad, ldw, net_W(n, td.comp), ldw, td.Do, td.Di, td.K, td.memo, c.darts_flags, td.share,
                                       c.darts_temp_proportion, 1.0f, net_Ag(n, td.comp), n->tapdots, s));
      if (!use_ng) {
        hipLaunchKernelGGL(add_scaled_taps_kernel, dim3(grid_for((long long)td.Do * ldw, 256)), dim3(256), 0, s, n->tapgrad, eff,
                           net_Wg(n, td.comp), td.Do, ldw, td.Di);
        if (!bias_done) TDNNF_HIP(colsum_add(view(dyv), 1.0f, net_Bg(n, td.comp), n->ws, s));
        return TDNNF_OK;
      }
    }
    // uniform-sample mode: only the share tap and the sampled tap are non-zero (:293-304) -> compacted launch
    const bool compact = td.darts && (c.darts_flags & TDNNF_DARTS_UNIFORM_SAMPLE) && td.K > 2;
    return param_grad(td.comp, td.ix, td.K, td.Di, td.Do, x, dyv, eff, bias_done, compact ? td.active : nullptr, compact ? 2 : 0, tap_ready);
  }

  int backward_heads() {
    if (!early_at_fork) CK(finish_refreshes());
    // Where in the host's order: minibatches whose GEMMs fill the chip start the statistics BEHIND the xent head's backward pass -- they then run
    // while the caller's stream waits for the denominator instead of beside the xent head's GEMMs (same step time, 124.0 against 124.1 ms, and the
    // 128 x 128 class is not slowed: 99.5 against 96.4 TFLOP/s, weight gradients 107 against 102); the small ones start them at once (behind the
    // xent head: 13.03 -> 13.10 ms at 150 x 64, 23.16 -> 23.31 at 1500 x 16).
    if (n->wg_on) CK(launch_early_in(2));
    for (int h = 1; h >= 0; h--) CK(backward_head(h));  // xent head first: it does not depend on the denominator
    CK(capture("prefinal-l.deriv", d_pl));
    CK(split(d_pl, 0, kP | kT, &po_dpl, s));
    {
      PlanesHintScope ph(hint_of(po_dpl), hint_of(po_top));
      CK(param_grad(n->c_prefinal_l, ix1, 1, Hd, S, &top, &d_pl, nullptr, false, nullptr, 0, false));
    }
    CK(close_bucket(-2));
    return phase_mark(n, 3, s);
  }
  int backward_head(int h) {
    auto &H = n->head[h];
    TraceRange trace_head(h == 0 ? "backward prefinal-chain / output" : "backward prefinal-xent / output-xent");
    if (h == 0) {
      // objective, part 3: join the denominator stream, d_y += posteriors, objf / failure handling
      TDNNF_HIP(hipStreamWaitEvent(s, n->ev_den, 0));
      den_joined = true;
      n->wg_two = n->wg_on && n->ws2 != nullptr;  // the denominator's stream is idle from here on
      CK(chain_finish(den, sup, &y, c.chain_l2_regularize, results, &dy, nullptr, n->chain_ws, s));
    }
    tdnnf_mat dout = h == 0 ? dy : dx;
    tdnnf_mat b2 = M(H.bn2_out, No, S), b1 = M(H.bn1_out, No, Hd);
    // (lag3: head h = 1 takes the buffers of the top layer (Ltop), h = 0 those of the layer below: free again by the time those layers write them)
    float *d_b1_buf = !lag3 ? n->dA : dC_of(h == 1 ? Ltop : Ltop - 1), *d_b2_buf = !lag3 ? n->d_small2 : n->dS[h == 1 ? 0 : 1];
    tdnnf_mat d_b2 = M(d_b2_buf, No, S), d_b1 = M(d_b1_buf, No, Hd);
    const std::string hname = h == 0 ? "prefinal-chain" : "prefinal-xent";
    if (h == 1) CK(capture("output-xent.deriv", dout));
    PlanesOperand po_d;  // the derivative matrix being propagated: planes where a GEMM reads it
    CK(split(dout, 0, kP | kT, &po_d, s));
    {
      PlanesHintScope ph(hint_of(po_d), hint_of(po_b2[h]));
      CK(param_grad(H.c_output, ix1, 1, S, P, &b2, &dout, nullptr, false, nullptr, 0, false));
    }
    {
      PlanesHintScope ph(hint_of(po_d), wplanes(H.c_output));
      CK(tdnnf_affine_backprop(&dout, net_W(n, H.c_output), S, S, &d_b2, s));
    }
    CK(capture(hname + ".batchnorm2.deriv", d_b2));
    if (cv) CK(tdnnf_batchnorm_test_backprop(&d_b2, H.bn2_memo + 2 * S, &d_b2, s));
    else CK(tdnnf_batchnorm_backprop(&b2, &d_b2, 1.0f, H.bn2_memo, &d_b2, n->ws, n->ws_bytes, s));  // -> d lin_out
    CK(capture(hname + ".linear.deriv", d_b2));
    CK(split(d_b2, 0, kP | kT, &po_d, s));
    {
      PlanesHintScope ph(hint_of(po_d), hint_of(po_b1[h]));
      CK(param_grad(H.c_linear, ix1, 1, Hd, S, &b1, &d_b2, nullptr, false, nullptr, 0, false));
    }
    {
      PlanesHintScope ph(hint_of(po_d), wplanes(H.c_linear));
      CK(tdnnf_affine_backprop(&d_b2, net_W(n, H.c_linear), Hd, Hd, &d_b1, s));
    }
    CK(capture(hname + ".batchnorm1.deriv", d_b1));
    FroBound fb_d;
    CK(bn_relu_backward(H.aff_relu, d_b1, d_b1, 0, H.bn1_memo, H.relu_stats, bias_target(H.c_affine), H.c_affine, c.num_layers + 1 + h, nullptr, &fb_d,
                        &po_d));  // in place -> d affine out
    CK(capture(hname + ".affine.deriv", d_b1));
    if (!po_d.base || po_d.base != d_b1.data) CK(split(d_b1, 0, kP | kT, &po_d, s, fb_d));
    {
      PlanesHintScope ph(hint_of(po_d), hint_of(po_pl));
      CK(param_grad(H.c_affine, ix1, 1, S, Hd, &pl, &d_b1, nullptr, true, nullptr, 0, false));
    }
    PlanesHintScope ph_bp(hint_of(po_d), wplanes(H.c_affine));
    if (h == 1) {
      CK(tdnnf_affine_backprop(&d_b1, net_W(n, H.c_affine), S, S, &d_pl, s));
      if (!n->wg_on) CK(launch_early_in(early_at_fork ? 1 : 2));
    } else {
      tdnnf_mat tmp = M(!lag3 ? n->d_small2 : n->dS[0], No, S);  // (lag3: the xent head's d_b2 buffer -- its reader, three components back, has been waited for)
      CK(tdnnf_affine_backprop(&d_b1, net_W(n, H.c_affine), S, S, &tmp, s));
      CK(tdnnf_add_scaled(&tmp, 1.0f, &d_pl, s));
    }
    return TDNNF_OK;
  }
  int backward_trunk() {
    {
      tdnnf_mat d_top = M(d_cur, No, Hd);
      PlanesHintScope ph(hint_of(po_dpl), wplanes(n->c_prefinal_l));
      CK(tdnnf_affine_backprop(&d_pl, net_W(n, n->c_prefinal_l), Hd, Hd, &d_top, s));
    }
    for (int l = c.num_layers - 1; l >= 0; l--) CK(backward_layer(l));
    {  // tdnn1: batchnorm -> relu -> affine (the lda layer is fixed: no input derivative needed)
      FroBound fb_d;
      PlanesOperand po_d;
      tdnnf_mat d_aff = M(d_cur, N0, Hd);
      CK(bn_relu_backward(n->t1_relu, d_aff, d_aff, 0, n->t1_bn_memo, n->t1_relu_stats, bias_target(n->tdnn1.comp), n->tdnn1.comp, 0, mask_of(0), &fb_d, &po_d));
      if (!po_d.base) CK(split(d_aff, 0, kT, &po_d, s, fb_d));
      PlanesHintScope ph(hint_of(po_d), hint_of(po_lda));
      CK(param_grad(n->tdnn1.comp, ix1, 1, lda_dim, Hd, &lda_out, &d_aff, nullptr, true, nullptr, 0, false));
    }
    CK(close_bucket(-1));
    return phase_mark(n, 4, s);
  }
  int backward_layer(int l) {
    TdnnfLayer &L = n->layers[l];
    float *in_act = l > 0 ? n->layers[l - 1].noop_out : n->t1_bn;
    const int no = L.aff.rows_out, nl = L.lin.rows_out, ni = N_of(L.gin, B);
    // d_cur is needed again for the bypass term, so the derivative w.r.t. the affine output goes to dC
    tdnnf_mat d_out = M(d_cur, no, Hd), d_aff = M(dC_of(l), no, Hd);
    const std::string lname = "tdnnf" + std::to_string(l + 2);
    TraceRange trace_layer(("backward " + lname).c_str());
    CK(capture(lname + ".noop.deriv", d_out));
    FroBound fb_daff;
    PlanesOperand po_daff, po_dlin;
    CK(bn_relu_backward(L.relu_out, d_out, d_aff, max_off(L.aff), L.bn_memo, L.relu_stats, bias_target(L.aff.comp), L.aff.comp, 1 + l, mask_of(l + 1), &fb_daff,
                        &po_daff));
    CK(capture(lname + ".affine.deriv", d_aff));
    tdnnf_mat lin = M(L.lin_out, nl, L.bn);
    tdnnf_mat aff_in = L.perm ? M(L.lin_perm, nl, L.bn) : (L.c_arch >= 0 ? M(L.lin_masked, nl, L.bn) : lin);
    const float *lin_eff = L.lin.darts ? L.lin.memo + TDNNF_MAX_OFFSETS : nullptr;
    const float *aff_eff = L.aff.darts ? L.aff.memo + TDNNF_MAX_OFFSETS : nullptr;
    ProfFlopsScale taps_active(L.lin.darts && (c.darts_flags & TDNNF_DARTS_UNIFORM_SAMPLE) && L.lin.K > 2 ? 2.0 / L.lin.K : 1.0);
    if (pl_on && !po_daff.base) CK(split(d_aff, max_off(L.aff), kP | kT, &po_daff, s, fb_daff));
    {
      PlanesHintScope ph(hint_of(po_daff), hint_of(po_lin[l]));
      CK(tdnn_wgrad(L.aff, &aff_in, &d_aff, aff_eff, true));
    }
    PlanesHintScope ph_aff_bp(hint_of(po_daff), wplanes(L.aff.comp));  // (for the backward-data GEMM of the affine, either branch below)
    // (lag3: the matrix the .linear's gradient reads lives in this layer's dS buffer; with rho > 1 that is the un-permuted copy)
    // (and the permuted matrix is formed in d_small2: d_small still holds prefinal-l's output derivative, which its gradient may be reading)
    tdnnf_mat d_lin = M(lag3 ? (L.perm ? n->d_small2 : dS_of(l)) : n->d_small, nl, L.bn);
    if (L.perm) {  // rho > 1: some row classes receive no tap -> zero first, then add; un-permute afterwards
      TDNNF_HIP(hipMemsetAsync(d_lin.data, 0, sizeof(float) * (size_t)nl * d_lin.stride, s));
      CK(tdnnf_tdnn_backprop_data(&L.aff.ix, &d_aff, net_W(n, L.aff.comp), L.aff.K * L.bn, Hd, L.bn, aff_eff, &d_lin, s));
      tdnnf_mat un = M(lag3 ? dS_of(l) : n->d_small2, nl, L.bn);
      CK(tdnnf_reorder_rows(&d_lin, B, L.aff.ix.row_stride, 0, &un, s));
      d_lin = un;
    } else {
      CK(tdnn_backprop_data_impl(&L.aff.ix, &d_aff, net_W(n, L.aff.comp), L.aff.K * L.bn, Hd, L.bn, aff_eff, 1, nullptr, 0.f, 0, &d_lin, s));
    }
    if (L.c_arch >= 0) {
      // d_lin is the derivative w.r.t. the masked blocks: the CopyN factor receives colsum(lin * d) (-> gradient of the
      // C-vector), the linear output receives d * mask (ElementwiseProductComponent::Backprop :276-299)
      const int chunks = (nl + 511) / 512;
      hipLaunchKernelGGL(colsum_prod_partial_kernel, dim3((L.bn + 255) / 256, chunks), dim3(256), 0, s, view(&lin), view(&d_lin), 512, (float *)n->ws);
      hipLaunchKernelGGL(bn_choice_backward_kernel, dim3(1), dim3(256), 0, s, bn_choice(c), (const float *)n->ws, chunks, L.arch_p, net_Wg(n, L.c_arch));
      hipLaunchKernelGGL(col_scale_kernel, dim3(grid_for((long long)nl * L.bn, 256)), dim3(256), 0, s, view(&d_lin), L.arch_mask, view(&d_lin));
    }
    CK(capture(lname + ".linear.deriv", d_lin));
    tdnnf_mat in = M(in_act, ni, Hd);
    // (the never-added bias of a DARTS .linear is still updated by the reference, :614 -- Bg() is null for plain layers)
    if (pl_on) CK(split(d_lin, max_off(L.lin), kP | kT, &po_dlin, s));
    {
      PlanesHintScope ph(hint_of(po_dlin), hint_of(po_in[l]));
      CK(tdnn_wgrad(L.lin, &in, &d_lin, lin_eff, false));
    }
    CK(close_bucket(l));
    PlanesHintScope ph_lin_bp(hint_of(po_dlin), wplanes(L.lin.comp));  // (the backward-data GEMM of the linear below)
    // deriv w.r.t. the layer input = linear backprop (overwrites) + bypass_scale * d_out on the output-grid rows
    tdnnf_mat d_in = M(d_next, ni, Hd);
    tdnnf_mat d_byp = sub_grid_view(d_next, L.gin, L.gout, B, Hd);
    if (d_byp.rows == d_out.rows) {  // contiguous rows: fused into the GEMM epilogue
      const int row0 = (int)((d_byp.data - d_in.data) / d_in.stride);
      CK(tdnn_backprop_data_impl(&L.lin.ix, &d_lin, net_W(n, L.lin.comp), L.lin.K * Hd, L.bn, Hd, lin_eff, 1, &d_out, c.bypass_scale, row0,
                                 &d_in, s));
    } else {
      CK(tdnn_backprop_data_impl(&L.lin.ix, &d_lin, net_W(n, L.lin.comp), L.lin.K * Hd, L.bn, Hd, lin_eff, 1, nullptr, 0.f, 0, &d_in, s));
      tdnnf_mat d_o = tdnnf_mat{d_cur, L.gout.n, d_byp.cols, B * ldpad(Hd)};
      CK(tdnnf_add_scaled(&d_o, c.bypass_scale, &d_byp, s));
    }
    std::swap(d_cur, d_next);
    return TDNNF_OK;
  }
  int join() {
    if (n->wg_on) CK(wait_last_wgrads(s, 3));  // join the weight-gradient streams (all three the event ring can hold)
    n->wg_two = false;
    if (use_ng) {  // join the side stream: every bucket has been committed into grads
      TDNNF_HIP(hipEventRecord(n->ev_s3, n->s3));
      TDNNF_HIP(hipStreamWaitEvent(s, n->ev_s3, 0));
    }
    CK(phase_mark(n, 5, s));
    TDNNF_LAUNCH_CHECK();
    return TDNNF_OK;
  }

  int run() {
    CK(begin());
    BnSyncScope bn_sync_scope(n->bn_sync.fn && !c.cv_update ? &n->bn_sync : nullptr);  // synchronised BatchNorm (data-parallel callers)
    // scope values: 1 two bf16 planes split in the kernel, 3 three; 4 pre-split f16 pairs (exact f32 where no planes are hinted)
    GemmPrecisionScope gemm_arith(c.gemm_precision == 2 ? 3 : c.gemm_precision == 3 ? 4 : c.gemm_precision);
    CK(weight_planes());
    TransposedWeightsScope gemm_wt(n->params, n->paramsT, n->paramsT ? n->num_params : 0);
    CK(transpose_weights());
    TraceRange trace_step("tdnnf_net_forward_backward");
    CK(forward_trunk());
    CK(forward_heads_and_objective());
    CK(backward_heads());
    CK(backward_trunk());
    return join();
  }
  // tdnnf_net_objective: run() without begin() (the step count, the gradient scratch, the refresh uploads), the W^T transpose, the backward
  // phases and the join of the gradient streams
  int run_objective() {
    BnSyncScope bn_sync_scope(n->bn_sync.fn && !c.cv_update ? &n->bn_sync : nullptr);
    GemmPrecisionScope gemm_arith(c.gemm_precision == 2 ? 3 : c.gemm_precision == 3 ? 4 : c.gemm_precision);
    CK(weight_planes());
    size_t objf_bytes = tdnnf_chain_objf_workspace_bytes(den, B, n->Tout);
    TDNNF_REQUIRE(n->chain_ws_bytes >= objf_bytes, "net_objective: denominator graph changed size");
    TraceRange trace_step("tdnnf_net_objective");
    CK(forward_trunk());
    CK(forward_heads_and_objective());
    TDNNF_LAUNCH_CHECK();
    return TDNNF_OK;
  }
};

}  // namespace

extern "C" {

int tdnnf_net_forward_backward(tdnnf_net *n, const tdnnf_mat *feats, const tdnnf_mat *ivectors, const tdnnf_den_graph *den,
                               const tdnnf_supervision *sup, double *results, long long step, tdnnf_stream stream) {
  TDNNF_REQUIRE(n && n->params && n->grads, "net_forward_backward: call net_set_buffers first");
  TDNNF_REQUIRE(mat_ok(feats) && mat_ok(ivectors) && den && sup && results, "net_forward_backward: bad arguments");
  const tdnnf_net_config &c = n->cfg;
  TDNNF_REQUIRE(feats->rows == n->g_feat.n * n->B && feats->cols == c.feat_dim, "net_forward_backward: feats must be %d x %d (t-major)",
                n->g_feat.n * n->B, c.feat_dim);
  TDNNF_REQUIRE(ivectors->rows == n->B && ivectors->cols == c.ivector_dim, "net_forward_backward: ivectors must be %d x %d", n->B, c.ivector_dim);
  if (!n->chain_ws) CK(create_streams_and_events(n, den));
  return Step(n, feats, ivectors, den, sup, results, step, (hipStream_t)stream).run();
}

int tdnnf_net_objective(tdnnf_net *n, const tdnnf_mat *feats, const tdnnf_mat *ivectors, const tdnnf_den_graph *den, const tdnnf_supervision *sup,
                        double *results, int flags, tdnnf_stream stream) {
  TDNNF_REQUIRE(n && n->params, "net_objective: call net_set_buffers first");
  TDNNF_REQUIRE(mat_ok(feats) && mat_ok(ivectors) && den && sup && results, "net_objective: bad arguments");
  TDNNF_REQUIRE((flags & ~TDNNF_OBJECTIVE_STORE_BATCHNORM_STATS) == 0, "net_objective: unknown flags %d", flags);
  const tdnnf_net_config &c = n->cfg;
  TDNNF_REQUIRE(feats->rows == n->g_feat.n * n->B && feats->cols == c.feat_dim, "net_objective: feats must be %d x %d (t-major)", n->g_feat.n * n->B, c.feat_dim);
  TDNNF_REQUIRE(ivectors->rows == n->B && ivectors->cols == c.ivector_dim, "net_objective: ivectors must be %d x %d", n->B, c.ivector_dim);
  if (!n->chain_ws) CK(create_streams_and_events(n, den));
  return Step(n, feats, ivectors, den, sup, results, 0, (hipStream_t)stream, flags).run_objective();
}

int tdnnf_net_phase_times(tdnnf_net *n, double *ms_out, int capacity, int *count) {
  TDNNF_REQUIRE(n && ms_out && count && capacity >= tdnnf_net::kPhases - 1, "net_phase_times: bad arguments (capacity >= 7)");
  *count = 0;
  for (int k = 0; k < tdnnf_net::kPhases; k++)
    if (!n->phase_rec[k]) return TDNNF_OK;  // (option phase_events was off for the last step)
  TDNNF_HIP(hipEventSynchronize(n->ev_phase[tdnnf_net::kPhases - 1]));
  for (int k = 0; k + 1 < tdnnf_net::kPhases; k++) {
    float ms = 0.f;
    TDNNF_HIP(hipEventElapsedTime(&ms, n->ev_phase[k], n->ev_phase[k + 1]));
    ms_out[k] = ms;
  }
  *count = tdnnf_net::kPhases - 1;
  return TDNNF_OK;
}

}  // extern "C"
