// net_step_grad.hip -- a component's gradient inside a step (Step, net_step.h): where it is formed (the caller's stream or one of up to three
// weight-gradient streams, with the ring of events that lets the caller run ahead), param_grad itself (raw, or the natural-gradient passes
// and chain of ng.h), when a bucket of the flat gradient is final; then the natural-gradient scheduling around it: refresh uploads, the
// input-side statistics ahead of the backward pass, the output-side statistic fused into the BatchNorm / ReLU sweep, the grouped chain.
#include "net_step.h"

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
// grads += this minibatch's gradient, unless the chain objective failed (results[5] == 0): then, as in the
// reference (derivatives set to zero), the minibatch contributes nothing
__global__ void commit_grads_kernel(float *grads, const float *gtmp, long long n, const double *results) {
  if (results[5] == 0.0) return;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += gridDim.x * 256LL) grads[i] += gtmp[i];
}
}  // namespace

// `st` waits for the last component of each of the `streams` weight-gradient streams in use
int Step::wait_last_wgrads(hipStream_t st, unsigned streams) {
  for (unsigned b = 1; b <= streams && b <= n->pg_count; b++) TDNNF_HIP(hipStreamWaitEvent(st, n->ev_pg[(n->pg_count - b) & 3], 0));
  return TDNNF_OK;
}
float *Step::bias_target(int comp) const {  // where a fused backward pass should accumulate the raw bias gradient
  if (n->comps[comp].lr_factor == 0.f) return nullptr;  // "if (to_update && learning_rate != 0)": no model derivative
  if (!use_ng) return net_Bg(n, comp);
  return n->ngc[comp].bsum;  // (zeroed with all the others at the start of the step)
}
// Where the next component's gradient is formed, with the workspace and the split-K scratch that go with the stream.
// Small minibatches: the weight-gradient side (gradient GEMM + slab reduce + the natural-gradient passes of the component) is the longer
// chain of the two -- 216 us per component against 145 on the caller's stream at 150 x 64 -- and the caller may only run one component
// ahead of it.  From the denominator's join on its stream is idle: components alternate between the two (event parity = stream parity).
// Which of the weight-gradient streams: s4 [s5] before the denominator's join, s4 s2 [s5] in turn after it.
Step::WgradSide Step::wgrad_side(bool on_caller) const {
  if (!n->wg_on || on_caller) return {s, n->ws, nullptr};
  const int ns = (n->wg_two ? 2 : 1) + (n->s5 ? 1 : 0), k = (int)(n->pg_count % (unsigned)ns);
  if (k == 0) return {n->s4, n->ws4, n->s4_scratch};
  if (k == 1 && n->wg_two) return {n->s2, n->ws2, n->s2_scratch};
  return {n->s5, n->ws5, n->s5_scratch};
}
// after this component is enqueued (on sw) the caller's stream may only run ahead of it, not of the one before: what that one reads
// (derivative scratch, the bias sums) is rewritten from here on
int Step::handed_off(hipStream_t sw, bool on_caller) {
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
int Step::param_grad(int comp, const tdnnf_tdnn_indexes &ix, int K, int Di, int Do, tdnnf_mat *x, tdnnf_mat *dyv, const float *eff, bool bias_done,
                     const int *active, int max_active, bool from_tapgrad) {
  const int ldw = K * Di;
  float *bias_acc = net_Bg(n, comp);
  if (n->comps[comp].lr_factor == 0.f) return TDNNF_OK;  // frozen component (cv-update): the reference skips its update
  // (option wgrad_on_caller: the xent head's components -- before the denominator's join, with the input-side statistics of the whole net
  // queued on s4 in front of them -- form their gradients on the caller's stream, which waits for the denominator anyway)
  const bool on_caller = n->wg_on && options().wgrad_on_caller != 0 && n->early_any && !den_joined;
  if (on_caller) caller_used = true;
  // sw: where the gradient is formed -- a weight-gradient stream (its inputs are final on s now), or s itself
  const WgradSide side = wgrad_side(on_caller);
  const hipStream_t sw = side.st;
  void *const wsw = side.ws;
  if (n->wg_on && !on_caller) CK(record_wait(n->ev_pg_in, s, sw));
  SplitKScratchOverride sw_scratch(side.scratch, side.scratch ? n->s4_scratch_bytes : 0);
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
  } else {  // per-object chain (first minibatch): the R x R work, the projections of the raw gradient and the commit, on the side stream
    CK(record_wait(n->ev_ngc, sw, n->s3));
    SplitKScratchOverride side_scratch(n->s3_scratch, n->s3_scratch_bytes);
    CK(ng_chain_one(n->ng_in[comp], n->ng_out[comp], C.H_in, C.part_in, C.H_out, C.part_out, T, Do, Dx, ldT, ldw, net_Wg(n, comp), bias_acc,
                    n->ng_side_ws, n->ngset_ws_bytes, n->ngTmp, n->s3));
  }
  CK(handed_off(sw, on_caller));
  // (the unscaled tap gradients this one reads are rebuilt by the next DARTS component on the caller's stream)
  if (from_tapgrad && n->wg_on) TDNNF_HIP(hipStreamWaitEvent(s, n->ev_pg[(n->pg_count - 1) & 3], 0));
  return TDNNF_OK;
}
// the gradient of an untapped affine component (prefinal-l, the heads' three, tdnn1) from the planes of its two operands
int Step::affine_grad(int comp, const PlanesOperand &p_dy, const PlanesOperand &p_x, tdnnf_mat *x, tdnnf_mat *dyv, bool bias_done) {
  PlanesHintScope ph(hint_of(p_dy), hint_of(p_x));
  return param_grad(comp, ix1, 1, x->cols, dyv->cols, x, dyv, nullptr, bias_done, nullptr, 0, false);
}
// weight gradient of one Tdnn component.  DARTS in a non-sampling mode also needs the architecture-logit
// gradient (UpdateNaturalGradient :516-590): tap gradients are formed unscaled once, s_i = <dW_i, W_i>
// replaces the reference's extra forward GEMM per tap, then c_i * dW_i goes into the accumulator.  p_dy, p_x: the planes of the two operands.
int Step::tdnn_wgrad(Tdnn &td, const PlanesOperand &p_dy, const PlanesOperand &p_x, tdnnf_mat *x, tdnnf_mat *dyv, const float *eff, bool bias_done) {
  PlanesHintScope ph(hint_of(p_dy), hint_of(p_x));
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
  const bool compact = two_taps(td);
  return param_grad(td.comp, td.ix, td.K, td.Di, td.Do, x, dyv, eff, bias_done, compact ? td.active : nullptr, compact ? 2 : 0, tap_ready);
}
// A bucket of the flat gradient buffer is final once the last of its components (in backward order) has been enqueued:
// grads[range] += this minibatch's gradient (unless the objective failed), then the bucket's event.  With natural gradient
// the components' commits run on the side stream, so the bucket's commit follows them there.
int Step::close_bucket(int key) {
  if (use_ng) CK(ng_close(key));
  for (auto &gb : n->buckets) {
    if (gb.close_key != key) continue;
    hipStream_t cs = s;
    if (!use_ng && n->wg_on && n->pg_count > 0) CK(wait_last_wgrads(s, side_streams()));  // the components' gradients were formed on s4 (and s2)
    if (use_ng) {
      CK(record_wait(gb.handoff, s, n->s3));  // s-side writes of the range (bias sums, architecture parameters) are done
      cs = n->s3;
    }
    const long long cnt = gb.end - gb.begin;
    if (cnt > 0)
      hipLaunchKernelGGL(commit_grads_kernel, dim3(grid_for(cnt, 256)), dim3(256), 0, cs, n->grads + gb.begin, n->gtmp + gb.begin, cnt, results);
    TDNNF_HIP(hipEventRecord(gb.ready, cs));
  }
  return TDNNF_OK;
}

// ---------------------------------------------------------------- the natural-gradient scheduling
std::vector<tdnnf_ng *> Step::all_ng() const {
  std::vector<tdnnf_ng *> v;
  for (auto *list : {&n->ng_in, &n->ng_out})
    for (tdnnf_ng *g : *list)
      if (g) v.push_back(g);
  return v;
}
// Refreshes whose host part has finished: upload W_{t+1} now (begin), on the side stream, which is idle during the forward pass --
// otherwise the ~9 small launches of each (18 refreshes per step) sit in front of the component's statistics passes in the
// backward pass.  Whatever is not ready yet stays with its next use.
int Step::upload_ready_refreshes() {
  if (!(c.use_natural_gradient && n->s3)) return TDNNF_OK;
  CK(record_wait(n->ev_fin0, s, n->s3));
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
// pending refreshes, and the input-side statistics that need nothing but forward activations
int Step::finish_refreshes() {
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
bool Step::is_head_comp(int comp) const {
  return comp == n->c_prefinal_l || comp == n->head[0].c_affine || comp == n->head[0].c_linear || comp == n->head[0].c_output ||
         comp == n->head[1].c_affine || comp == n->head[1].c_linear || comp == n->head[1].c_output;
}
// input-side statistics of every component whose backward call of the previous minibatch recorded its arguments (and has not come yet
// in this one) and whose preconditioners exist (the grouped chain will take them): on s4, behind the forward pass and the refresh uploads
bool Step::early_eligible(int comp, int which) const {
  const auto &E = n->early[comp];
  if (E.done == n->fb_count || (which == 0 && is_head_comp(comp))) return false;
  if (E.recorded != n->fb_count - 1 || !n->ng_in[comp] || !n->ng_out[comp] || ng_dim(n->ng_in[comp]) == 0 || ng_dim(n->ng_out[comp]) == 0) return false;
  return n->comps[comp].lr_factor != 0.f && n->ngc[comp].H_in;
}
// which: 0 the trunk's components (their inputs exist once the trunk's forward pass is enqueued), 1 the heads' (and whatever was not launched yet), 2 all
int Step::launch_early_in(int which) {
  if (!(use_ng && n->early_on)) return TDNNF_OK;
  std::vector<int> who;
  for (int comp = (int)n->comps.size() - 1; comp >= 0; comp--)
    if (early_eligible(comp, which)) who.push_back(comp);
  if (who.empty()) return TDNNF_OK;
  CK(record_wait(n->ev_early_in, s, n->s4));
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
int Step::out_stats_fuse(int comp, MatView xv, MatView dzv, MatView dv, NgFuse &f) {  // 1: f is to be passed on
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
// Natural gradient, grouped: the chains of the components enqueued since the last bucket closed, as one sequence of grouped
// launches on the side stream behind their N-sized passes.
int Step::ng_close(int key) {
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
    if (caller_used) CK(record_wait(n->ev_ngc, s, n->s3));
    caller_used = false;
  } else {
    CK(record_wait(n->ev_ngc, s, n->s3));
  }
  if (n->early_any) TDNNF_HIP(hipStreamWaitEvent(n->s3, n->ev_early, 0));  // the H_in of this step (all of them: one event)
  CK(ng_group_run(nb->group, n->s3));
  n->ng_cur.clear();
  return TDNNF_OK;
}

}  // namespace tdnnf
