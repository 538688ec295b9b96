// net_step.hip -- one minibatch of nnet3-chain-train on a tdnnf_net (net.h): tdnnf_net_forward_backward, as a host-side C++
// executor over the component kernels of this library.
//
// Mirrors (UPSTREAM) NnetChainTrainer::TrainInternal:  forward through every component's Propagate,
// chain::ComputeChainObjfAndDeriv, Backprop through every component (raw-gradient / is_gradient_
// UpdateSimple path); the optimizer helpers that follow are tdnnf_net_update (net_update.hip).
//
// This unit is the schedule of the step object (Step, net_step.h, with the map of the units that define the rest of its methods): run() lists
// the phases between the phase_mark boundaries, the phases below it say what is enqueued where, in the order of the step.
#include <math.h>

#include "net_step.h"

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
}  // namespace

namespace tdnnf {
namespace {
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
}  // namespace

// Affine (+ bias) + ReLU of component `comp` (K taps) into `out` and the BatchNorm statistics of that output; the GEMM's epilogue forms the
// column sums while it stores the tile when it can (exact-f32 128-wide tile), otherwise a pass over `out` does.  The normalisation itself
// is applied later by a fused pass.  p_x: the planes of `in`; the BatchNorm finalize leaves the norm bound of `out` for *fb.
int Step::affine_relu_bn_stats(int comp, const tdnnf_tdnn_indexes *ix, int K, const PlanesOperand &p_x, const tdnnf_mat *in, const float *eff, tdnnf_mat *out,
                               float *memo, double *stats, FroBound *fb) {
  PlanesHintScope ph(hint_of(p_x), wplanes(comp));
  FroBoundScope fbs(pl_on ? n->fro_buf : nullptr, &fb->blocks);
  const float *W = net_W(n, comp), *bias = net_bias(n, comp);
  const int Di = in->cols, Do = out->cols, ldw = K * Di;
  if (cv) {
    CK(tdnn_propagate_impl(ix, in, W, ldw, Do, Di, bias, eff, 1, 1, out, s));
    return bn_test_memo(memo, stats, Do, s);
  }
  if (!store_bn) stats = nullptr;  // (bn_fwd)
  int prows = 0;
  const bool room = n->ws_bytes >= sizeof(float) * 2 * (size_t)Do * rows_gemm_colstats_cap(out->rows);
  CK(tdnn_propagate_impl(ix, in, W, ldw, Do, Di, bias, eff, 1, 1, out, s, room ? (float *)n->ws : nullptr, room ? &prows : nullptr));
  // (StoreStats runs on every minibatch: in the finalize launch)
  if (prows > 0) TDNNF_HIP(batchnorm_stats_from_partials((const float *)n->ws, prows, out->rows, Do, 1.0e-3f, 1.0f, memo, s, stats));
  else TDNNF_HIP(batchnorm_stats(view(out), 1.0e-3f, 1.0f, memo, n->ws, s, stats));
  return TDNNF_OK;
}
int Step::affine_forward(int comp, const PlanesOperand &p_x, tdnnf_mat *x, tdnnf_mat *yv) {
  PlanesHintScope ph(hint_of(p_x), wplanes(comp));
  return tdnnf_affine_propagate(x, net_W(n, comp), x->cols, net_bias(n, comp), yv->cols, yv, s);
}
int Step::affine_backward_data(int comp, const PlanesOperand &p_dy, tdnnf_mat *dyv, tdnnf_mat *dxv) {
  PlanesHintScope ph(hint_of(p_dy), wplanes(comp));
  return tdnnf_affine_backprop(dyv, net_W(n, comp), dxv->cols, dxv->cols, dxv, s);
}

// ---------------------------------------------------------------- the step
int Step::run() {
  CK(begin());
  BnSyncScope bn_sync_scope(n->bn_sync.fn && !c.cv_update ? &n->bn_sync : nullptr);  // synchronised BatchNorm (data-parallel callers)
  // scope values: 1 two bf16 planes split in the kernel, 3 three; 4 pre-split f16 pairs (exact f32 where no planes are hinted)
  GemmPrecisionScope gemm_arith(c.gemm_precision == 2 ? 3 : c.gemm_precision == 3 ? 4 : c.gemm_precision);
  CK(weight_planes());
  TransposedWeightsScope gemm_wt(n->params, n->paramsT, n->paramsT ? n->num_params : 0);
  CK(transpose_weights());
  TDNNF_REQUIRE(n->chain_ws_bytes >= tdnnf_chain_workspace_bytes(den, B, n->Tout) - (n->den_split ? 0 : chain_split_region_bytes(den, B, n->Tout)),
                "net_forward_backward: denominator graph changed size");
  TraceRange trace_step("tdnnf_net_forward_backward");
  CK(forward_trunk());
  CK(forward_heads_and_objective());
  CK(backward_heads());
  CK(backward_trunk());
  return join();
}
// tdnnf_net_objective: run() without begin() (the step count, the gradient scratch, the refresh uploads), the W^T transpose, the backward
// phases and the join of the gradient streams
int Step::run_objective() {
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

// ---------------------------------------------------------------- phases
int Step::begin() {
  n->fb_count++;
  CK(phase_mark(n, 0, s));
  n->wg_two = false;  // (a step that failed half-way may have left it set)
  TDNNF_HIP(hipMemsetAsync(n->gtmp, 0, sizeof(float) * (size_t)n->num_params, s));
  if (n->ng_bsum_all && n->ng_bsum_floats) TDNNF_HIP(hipMemsetAsync(n->ng_bsum_all, 0, sizeof(float) * n->ng_bsum_floats, s));  // every component's raw bias gradient
  n->pg_count = 0;
  n->early_any = false;
  n->ng_cur.clear();
  return upload_ready_refreshes();
}

// ================================================================= forward
int Step::forward_trunk() {
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
  CK(affine_relu_bn_stats(n->tdnn1.comp, &ix1, 1, po_lda, &lda_out, nullptr, &t1r, n->t1_bn_memo, n->t1_bn_stats, &fb_next));
  fb_next.mul = mask_max;
  CK(bn_apply_planes(t1r, n->t1_bn_memo, none, 0.f, t1b, mask_of(0), fb_next, &po_next));
  prev = n->t1_bn;
  int layer_no = 0;
  for (auto &L : n->layers) CK(forward_layer(L, ++layer_no));
  return mark(1);
}
int Step::forward_layer(TdnnfLayer &L, int layer_no) {
  TraceRange trace_layer(("forward tdnnf" + std::to_string(layer_no + 1)).c_str());
  PlanesOperand &p_in = po_in[layer_no - 1], &p_lin = po_lin[layer_no - 1];
  tdnnf_mat in = M(prev, N_of(L.gin, B), Hd);
  tdnnf_mat lin = M(L.lin_out, L.lin.rows_out, L.bn);
  const float *lin_eff = darts_eff(L.lin), *aff_eff = darts_eff(L.aff);
  if (L.lin.darts) {
    TDNNF_REQUIRE(n->draws, "net_forward_backward: a DARTS net needs net_set_random_draws before every step");
    if (!darts_coef_done) CK(darts_coef(n, L, s));
    if (pl_on && !darts_coef_done) {  // the effective coefficients folded into this step's weight planes
      CK(split_weights(L.lin.comp, lin_eff, Hd));
      CK(split_weights(L.aff.comp, aff_eff, L.bn));
    }
  }
  // uniform-sample mode runs at most two taps of K (share + sampled): tell the FLOP accounting of the profiler
  ProfFlopsScale taps_active(two_taps(L.lin) ? 2.0 / L.lin.K : 1.0);
  // (DARTS .linear: bias present but offsets[1] < 0 -> out is zeroed and the bias never added, :237-240)
  if (pl_on) CK(next_input_planes(in, &p_in));  // (the planes are also the tile-row operand of this layer's weight gradient)
  fb_next = FroBound();
  po_next = PlanesOperand();
  {
    PlanesHintScope ph(hint_of(p_in), wplanes(L.lin.comp));
    CK(tdnnf_tdnn_propagate(&L.lin.ix, &in, net_W(n, L.lin.comp), L.lin.K * Hd, L.bn, Hd, nullptr, lin_eff, 2, &lin, s));
  }
  tdnnf_mat aff_in = lin;
  if (L.c_arch >= 0) {  // bottleneck supernet: column blocks of the linear output times CopyN(Sum(p_k..))
    CK(bn_choice_forward(n, L, s));
    aff_in = M(L.lin_masked, L.lin.rows_out, L.bn);
  }
  if (L.perm) {
    tdnnf_mat src = aff_in;
    aff_in = M(L.lin_perm, L.lin.rows_out, L.bn);
    CK(tdnnf_reorder_rows(&src, B, L.aff.ix.row_stride, 1, &aff_in, s));
  }
  tdnnf_mat relu = M(L.relu_out, L.aff.rows_out, Hd);
  if (pl_on && !L.perm) CK(split(aff_in, 0, kP | kT, &p_lin, s));  // (the linear output, or its masked blocks in the bottleneck supernet)
  CK(affine_relu_bn_stats(L.aff.comp, &L.aff.ix, L.aff.K, p_lin, &aff_in, aff_eff, &relu, L.bn_memo, L.bn_stats, &fb_next));
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

int Step::forward_heads_and_objective() {
  if (early_at_fork && !objective) {
    CK(finish_refreshes());
    CK(launch_early_in(0));
  }
  top = M(prev, No, Hd);
  CK(next_input_planes(top, &po_top));
  CK(affine_forward(n->c_prefinal_l, po_top, &top, &pl));
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
int Step::forward_head(int h) {
  auto &H = n->head[h];
  tdnnf_mat ar = M(H.aff_relu, No, Hd), lo = M(H.lin_out, No, S), b1 = M(H.bn1_out, No, Hd), b2 = M(H.bn2_out, No, S), yh = M(H.y, No, P);
  FroBound fb_b1;
  CK(affine_relu_bn_stats(H.c_affine, &ix1, 1, po_pl, &pl, nullptr, &ar, H.bn1_memo, H.bn1_stats, &fb_b1));
  CK(bn_apply_planes(ar, H.bn1_memo, none, 0.f, b1, nullptr, fb_b1, &po_b1[h]));
  if (!po_b1[h].base) CK(split(b1, 0, kP | kT, &po_b1[h], s, fb_b1));
  CK(affine_forward(H.c_linear, po_b1[h], &b1, &lo));
  CK(bn_fwd(n, H.lin_out, H.bn2_out, No, S, H.bn2_memo, H.bn2_stats, s, store_bn));
  CK(split(b2, 0, kP | kT, &po_b2[h], s));
  return affine_forward(H.c_output, po_b2[h], &b2, &yh);
}
// ====================================================== objective, part 1 (second stream)
// The denominator forward-backward (one workgroup per sequence) only needs the chain head's output: it
// runs on n->s2 while this stream does the xent head forward, the numerator and the xent head backward.
int Step::fork_objective() {
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
int Step::fork_objective_only() {
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
int Step::capture(const std::string &name, const tdnnf_mat &m) {
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
// NonlinearComponent::StoreBackpropStats (nnet-component-itf.cc:461-480): "if (RandInt(0, 3) == 0 && oderiv_count_ != 0) return"
// -- three minibatches in four, always the first; a decision stream of its own (the k-th ReLU of the backward pass)
double *Step::oderiv_of(double *relu_stats, int relu_index) {  // relu_index: the k-th ReLU of stat_blocks() (net_model.h); every ReLU is Hd wide
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
int Step::bn_relu_backward(float *relu_out, const tdnnf_mat &d_in, const tdnnf_mat &d_out, int lead, float *memo, double *relu_stats, float *bias_acc, int comp,
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
int Step::backward_heads() {
  if (!early_at_fork) CK(finish_refreshes());
  // Where in the host's order: minibatches whose GEMMs fill the chip start the statistics BEHIND the xent head's backward pass -- they then run
  // while the caller's stream waits for the denominator instead of beside the xent head's GEMMs (same step time, 124.0 against 124.1 ms, and the
  // 128 x 128 class is not slowed: 99.5 against 96.4 TFLOP/s, weight gradients 107 against 102); the small ones start them at once (behind the
  // xent head: 13.03 -> 13.10 ms at 150 x 64, 23.16 -> 23.31 at 1500 x 16).
  if (n->wg_on) CK(launch_early_in(2));
  for (int h = 1; h >= 0; h--) CK(backward_head(h));  // xent head first: it does not depend on the denominator
  CK(capture("prefinal-l.deriv", d_pl));
  CK(split(d_pl, 0, kP | kT, &po_dpl, s));
  CK(affine_grad(n->c_prefinal_l, po_dpl, po_top, &top, &d_pl, false));
  CK(close_bucket(-2));
  return phase_mark(n, 3, s);
}
int Step::backward_head(int h) {
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
  CK(affine_grad(H.c_output, po_d, po_b2[h], &b2, &dout, false));
  CK(affine_backward_data(H.c_output, po_d, &dout, &d_b2));
  CK(capture(hname + ".batchnorm2.deriv", d_b2));
  if (cv) CK(tdnnf_batchnorm_test_backprop(&d_b2, H.bn2_memo + 2 * S, &d_b2, s));
  else CK(tdnnf_batchnorm_backprop(&b2, &d_b2, 1.0f, H.bn2_memo, &d_b2, n->ws, n->ws_bytes, s));  // -> d lin_out
  CK(capture(hname + ".linear.deriv", d_b2));
  CK(split(d_b2, 0, kP | kT, &po_d, s));
  CK(affine_grad(H.c_linear, po_d, po_b1[h], &b1, &d_b2, false));
  CK(affine_backward_data(H.c_linear, po_d, &d_b2, &d_b1));
  CK(capture(hname + ".batchnorm1.deriv", d_b1));
  FroBound fb_d;
  CK(bn_relu_backward(H.aff_relu, d_b1, d_b1, 0, H.bn1_memo, H.relu_stats, bias_target(H.c_affine), H.c_affine, c.num_layers + 1 + h, nullptr, &fb_d,
                      &po_d));  // in place -> d affine out
  CK(capture(hname + ".affine.deriv", d_b1));
  if (!po_d.base || po_d.base != d_b1.data) CK(split(d_b1, 0, kP | kT, &po_d, s, fb_d));
  CK(affine_grad(H.c_affine, po_d, po_pl, &pl, &d_b1, true));
  if (h == 1) {
    CK(affine_backward_data(H.c_affine, po_d, &d_b1, &d_pl));
    if (!n->wg_on) CK(launch_early_in(early_at_fork ? 1 : 2));
  } else {
    tdnnf_mat tmp = M(!lag3 ? n->d_small2 : n->dS[0], No, S);  // (lag3: the xent head's d_b2 buffer -- its reader, three components back, has been waited for)
    CK(affine_backward_data(H.c_affine, po_d, &d_b1, &tmp));
    CK(tdnnf_add_scaled(&tmp, 1.0f, &d_pl, s));
  }
  return TDNNF_OK;
}
int Step::backward_trunk() {
  tdnnf_mat d_top = M(d_cur, No, Hd);
  CK(affine_backward_data(n->c_prefinal_l, po_dpl, &d_pl, &d_top));
  for (int l = c.num_layers - 1; l >= 0; l--) CK(backward_layer(l));
  {  // tdnn1: batchnorm -> relu -> affine (the lda layer is fixed: no input derivative needed)
    FroBound fb_d;
    PlanesOperand po_d;
    tdnnf_mat d_aff = M(d_cur, N0, Hd);
    CK(capture("tdnn1.batchnorm.deriv", d_aff));
    CK(bn_relu_backward(n->t1_relu, d_aff, d_aff, 0, n->t1_bn_memo, n->t1_relu_stats, bias_target(n->tdnn1.comp), n->tdnn1.comp, 0, mask_of(0), &fb_d, &po_d));
    CK(capture("tdnn1.affine.deriv", d_aff));
    if (!po_d.base) CK(split(d_aff, 0, kT, &po_d, s, fb_d));
    CK(affine_grad(n->tdnn1.comp, po_d, po_lda, &lda_out, &d_aff, true));
  }
  CK(close_bucket(-1));
  return phase_mark(n, 4, s);
}
int Step::backward_layer(int l) {
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
  const float *lin_eff = darts_eff(L.lin), *aff_eff = darts_eff(L.aff);
  ProfFlopsScale taps_active(two_taps(L.lin) ? 2.0 / L.lin.K : 1.0);
  if (pl_on && !po_daff.base) CK(split(d_aff, max_off(L.aff), kP | kT, &po_daff, s, fb_daff));
  CK(tdnn_wgrad(L.aff, po_daff, po_lin[l], &aff_in, &d_aff, aff_eff, true));
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
  if (L.c_arch >= 0) CK(bn_choice_backward(n, L, d_lin, s));  // d_lin: from the derivative w.r.t. the masked blocks to that w.r.t. the linear output
  CK(capture(lname + ".linear.deriv", d_lin));
  tdnnf_mat in = M(in_act, ni, Hd);
  // (the never-added bias of a DARTS .linear is still updated by the reference, :614 -- Bg() is null for plain layers)
  if (pl_on) CK(split(d_lin, max_off(L.lin), kP | kT, &po_dlin, s));
  CK(tdnn_wgrad(L.lin, po_dlin, po_in[l], &in, &d_lin, lin_eff, false));
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
int Step::join() {
  if (n->wg_on) CK(wait_last_wgrads(s, 3));  // join the weight-gradient streams (all three the event ring can hold)
  n->wg_two = false;
  if (use_ng) CK(record_wait(n->ev_s3, n->s3, s));  // join the side stream: every bucket has been committed into grads
  CK(phase_mark(n, 5, s));
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

}  // namespace tdnnf

namespace {
// what both entries check, in this order, under the entry's name `who`; then the first step of a net creates its streams and events
int enter(const char *who, tdnnf_net *n, bool needs_grads, int flags, const tdnnf_mat *feats, const tdnnf_mat *ivectors, const tdnnf_den_graph *den,
          const tdnnf_supervision *sup, const double *results) {
  TDNNF_REQUIRE(n && n->params && (n->grads || !needs_grads), "%s: call net_set_buffers first", who);
  TDNNF_REQUIRE(mat_ok(feats) && mat_ok(ivectors) && den && sup && results, "%s: bad arguments", who);
  TDNNF_REQUIRE((flags & ~TDNNF_OBJECTIVE_STORE_BATCHNORM_STATS) == 0, "%s: unknown flags %d", who, flags);
  TDNNF_REQUIRE(!chain_supervision_needs_assign(sup), "%s: the reserved supervision holds no minibatch yet (tdnnf_supervision_assign gives it one)", who);
  const tdnnf_net_config &c = n->cfg;
  TDNNF_REQUIRE(feats->rows == n->g_feat.n * n->B && feats->cols == c.feat_dim, "%s: feats must be %d x %d (t-major)", who, n->g_feat.n * n->B, c.feat_dim);
  TDNNF_REQUIRE(ivectors->rows == n->B && ivectors->cols == c.ivector_dim, "%s: ivectors must be %d x %d", who, n->B, c.ivector_dim);
  if (!n->chain_ws) CK(create_streams_and_events(n, den));
  return TDNNF_OK;
}
}  // namespace

extern "C" {

int tdnnf_net_forward_backward(tdnnf_net *n, const tdnnf_mat *feats, const tdnnf_mat *ivectors, const tdnnf_den_graph *den,
                               const tdnnf_supervision *sup, double *results, long long step, tdnnf_stream stream) {
  CK(enter("net_forward_backward", n, true, 0, feats, ivectors, den, sup, results));
  return Step(n, feats, ivectors, den, sup, results, step, (hipStream_t)stream).run();
}

int tdnnf_net_objective(tdnnf_net *n, const tdnnf_mat *feats, const tdnnf_mat *ivectors, const tdnnf_den_graph *den, const tdnnf_supervision *sup,
                        double *results, int flags, tdnnf_stream stream) {
  CK(enter("net_objective", n, false, flags, feats, ivectors, den, sup, results));
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
