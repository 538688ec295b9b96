// net_create.hip -- the tdnnf_net object: creation (describe: net_graph.hip; allocate: the preconditioners, the bucket events and the
// arena of net_arena.hip; name), destruction, the accessors and setters of the C-ABI, and the statistics get / set.  The streams and the
// step's events are created by create_streams_and_events, which the net's first step calls (net_step.hip), not by create.
#include <string.h>

#include <string>
#include <vector>

#include "common.h"
#include "gemm_f32.h"
#include "net_model.h"
#include "ng.h"
#include "optim_group.h"

using namespace tdnnf;

namespace {

// the resources of a described net.  Any failure leaves a net that tdnnf_net_destroy takes apart.
int allocate(tdnnf_net *n, const tdnnf_net *share) {
  n->owns_ng = share == nullptr;
  if (share) {  // the primary's preconditioners
    n->ng_in = share->ng_in;
    n->ng_out = share->ng_out;
    n->oderiv_nonzero = share->oderiv_nonzero;
  } else if (n->cfg.use_natural_gradient) {
    // one input-side and one output-side preconditioner per updatable component
    n->ng_in.assign(n->comps.size(), nullptr);
    n->ng_out.assign(n->comps.size(), nullptr);
    for (size_t i = 0; i < n->comps.size(); i++) {
      const CompDesc &cd = n->comps[i];
      if (!cd.updatable || cd.plain) continue;  // fixed lda layer; vectors updated without natural gradient
      int rank_in, rank_out;
      ng_ranks(cd, &rank_in, &rank_out);
      CK(tdnnf_ng_create(rank_in, kNgUpdatePeriod, kNgNumSamplesHistory, kNgAlpha, &n->ng_in[i]));
      CK(tdnnf_ng_create(rank_out, kNgUpdatePeriod, kNgNumSamplesHistory, kNgAlpha, &n->ng_out[i]));
    }
  }
  for (auto &gb : n->buckets)
    if (hipEventCreateWithFlags(&gb.ready, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&gb.handoff, hipEventDisableTiming) != hipSuccess) {
      set_error("net_create: cannot create events");
      return TDNNF_EHIP;
    }
  Arena sizing;
  net_layout_arena(n, sizing);
  n->arena_bytes = sizing.off + 1024;
  if (hipMalloc((void **)&n->arena, n->arena_bytes) != hipSuccess) {
    set_error("net_create: cannot allocate %zu bytes of activations", n->arena_bytes);
    return TDNNF_EHIP;
  }
  hipMemset(n->arena, 0, n->arena_bytes);
  Arena real;
  real.base = n->arena;
  net_layout_arena(n, real);
  if (share) {  // the model's BatchNorm / ReLU statistics live in the primary net
    const std::vector<StatBlock> mine = stat_blocks(n), theirs = stat_blocks(share);
    for (size_t i = 0; i < mine.size(); i++) *mine[i].slot = theirs[i].p();
  }
  return TDNNF_OK;
}

int net_create_impl(const tdnnf_net_config *cfg, const tdnnf_net *share, tdnnf_net **out) {
  TDNNF_REQUIRE(cfg && out, "net_create: null argument");
  CK(net_check_config(*cfg));
  tdnnf_net *n = new tdnnf_net();
  n->cfg = *cfg;
  int rc = net_describe(n);
  if (!rc && share) rc = net_same_model(n, share);
  if (!rc) rc = allocate(n, share);
  if (rc) {
    tdnnf_net_destroy(n);
    return rc;
  }
  net_name_activations(n);
  *out = n;
  return TDNNF_OK;
}

// NameMatchesPattern (UPSTREAM, used by every edit directive of nnet-utils.cc:1166-1415): '*' matches any run of characters
bool name_matches(const char *name, const char *pat) {
  if (*pat == 0) return *name == 0;
  if (*pat == '*') {
    for (const char *p = name;; p++) {
      if (name_matches(p, pat + 1)) return true;
      if (*p == 0) return false;
    }
  }
  return *name == *pat && name_matches(name + 1, pat + 1);
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

}  // namespace

// the first step of a net: the chain workspace and every stream and event of the step, in this order (HIP maps streams to hardware
// queues in creation order); tdnnf_net_destroy below takes them apart
int tdnnf::create_streams_and_events(tdnnf_net *n, const tdnnf_den_graph *den) {
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

extern "C" {

int tdnnf_net_create(const tdnnf_net_config *cfg, tdnnf_net **out) { return net_create_impl(cfg, nullptr, out); }

int tdnnf_net_create_shared(const tdnnf_net_config *cfg, const tdnnf_net *primary, tdnnf_net **out) {
  TDNNF_REQUIRE(primary, "net_create_shared: null primary net");
  return net_create_impl(cfg, primary, out);
}

// (safe on a half-built net: every field starts null, net.h, and every destroy helper below takes a null)
void tdnnf_net_destroy(tdnnf_net *n) {
  if (!n) return;
  if (n->s3) hipStreamSynchronize(n->s3);  // its kernels use the preconditioners' buffers
  if (n->s4) hipStreamSynchronize(n->s4);
  if (n->s5) hipStreamSynchronize(n->s5);
  if (n->s2) hipStreamSynchronize(n->s2);
  for (auto &nb : n->ng_buckets) ng_group_destroy(nb.group);
  ng_fin_destroy(n->ngfin);
  if (n->ev_ngc) hipEventDestroy(n->ev_ngc);
  if (n->owns_ng) {
    for (auto *g : n->ng_in) tdnnf_ng_destroy(g);
    for (auto *g : n->ng_out) tdnnf_ng_destroy(g);
  }
  hipFree(n->arena);
  hipFree(n->chain_ws);
  for (float *p : n->captured) hipFree(p);
  for (auto &gb : n->buckets) {
    if (gb.ready) hipEventDestroy(gb.ready);
    if (gb.handoff) hipEventDestroy(gb.handoff);
  }
  if (n->s2) hipStreamDestroy(n->s2);
  if (n->ev_fork) hipEventDestroy(n->ev_fork);
  if (n->ev_den) hipEventDestroy(n->ev_den);
  if (n->ev_num) hipEventDestroy(n->ev_num);
  if (n->ev_s3) hipEventDestroy(n->ev_s3);
  if (n->ev_fin0) hipEventDestroy(n->ev_fin0);
  if (n->ev_fin) hipEventDestroy(n->ev_fin);
  if (n->s3) hipStreamDestroy(n->s3);
  for (hipEvent_t e : {n->ev_pg[0], n->ev_pg[1], n->ev_pg[2], n->ev_pg[3], n->ev_pg_in, n->ev_early_in, n->ev_early, n->ev_comm, n->ev_den_rec})
    if (e) hipEventDestroy(e);
  if (n->s4) hipStreamDestroy(n->s4);
  if (n->s5) hipStreamDestroy(n->s5);
  rows_gemm_group_destroy(n->early_launch);
  planes_split_group_destroy(n->wsplit_group);
  for (hipEvent_t e : n->ev_phase)
    if (e) hipEventDestroy(e);
  upd_group_destroy(n->upd);
  delete n;
}

long long tdnnf_net_num_params(const tdnnf_net *n) { return n ? n->num_params : 0; }
int tdnnf_net_num_components(const tdnnf_net *n) { return n ? (int)n->comps.size() : 0; }

int tdnnf_net_component_info(const tdnnf_net *n, int i, char *name_out, long long *begin, int *rows, int *cols, int *has_bias,
                             float *lr_factor, float *l2, float *max_change, float *orthonormal) {
  TDNNF_REQUIRE(n && i >= 0 && i < (int)n->comps.size(), "net_component_info: bad index");
  const CompDesc &c = n->comps[i];
  if (name_out) snprintf(name_out, 64, "%s", c.name.c_str());
  if (begin) *begin = c.begin;
  if (rows) *rows = c.rows;
  if (cols) *cols = c.cols;
  if (has_bias) *has_bias = c.has_bias;
  if (lr_factor) *lr_factor = c.lr_factor;
  if (l2) *l2 = c.l2;
  if (max_change) *max_change = c.max_change;
  if (orthonormal) *orthonormal = c.orthonormal;
  return TDNNF_OK;
}

// ---- model statistics outside the parameter vector, block after block in the order of stat_blocks() (net_model.h)
long long tdnnf_net_stats_size(const tdnnf_net *n) {
  if (!n) return 0;
  long long t = 0;
  for (const StatBlock &b : stat_blocks(n)) t += b.doubles();
  return t;
}
int tdnnf_net_get_stats(const tdnnf_net *n, double *host_out, tdnnf_stream stream) {
  TDNNF_REQUIRE(n && host_out, "net_get_stats: null argument");
  TDNNF_HIP(hipStreamSynchronize((hipStream_t)stream));
  for (const StatBlock &b : stat_blocks(n)) {
    TDNNF_HIP(hipMemcpy(host_out, b.p(), sizeof(double) * b.doubles(), hipMemcpyDeviceToHost));
    host_out += b.doubles();
  }
  return TDNNF_OK;
}
int tdnnf_net_set_stats(tdnnf_net *n, const double *host_in, tdnnf_stream stream) {
  TDNNF_REQUIRE(n && host_in, "net_set_stats: null argument");
  const std::vector<StatBlock> blocks = stat_blocks(n);
  std::vector<char> &nz = *n->oderiv_nonzero;  // (a shared net's is the primary's)
  nz.clear();
  const double *p = host_in;
  for (const StatBlock &b : blocks) {
    if (b.relu) nz.push_back(p[relu_oderiv_at(b.D)] != 0.0);
    p += b.doubles();
  }
  TDNNF_HIP(hipStreamSynchronize((hipStream_t)stream));
  for (const StatBlock &b : blocks) {
    TDNNF_HIP(hipMemcpy(b.p(), host_in, sizeof(double) * b.doubles(), hipMemcpyHostToDevice));
    host_in += b.doubles();
  }
  return TDNNF_OK;
}

int tdnnf_net_set_dropout_proportion(tdnnf_net *n, float proportion) {
  TDNNF_REQUIRE(n && proportion >= 0.f && proportion <= 0.5f, "net_set_dropout_proportion: proportion must be in [0, 0.5] (continuous masks: scale in [1 - 2p, 1 + 2p])");
  TDNNF_REQUIRE(proportion == 0.f || n->dropout_masks, "net_set_dropout_proportion: the net was created without use_dropout (or in cv-update mode)");
  n->dropout_proportion = proportion;
  return TDNNF_OK;
}

int tdnnf_net_set_temperature_proportion(tdnnf_net *n, float proportion) {
  TDNNF_REQUIRE(n && proportion > 0.f, "net_set_temperature_proportion: proportion must be > 0");
  n->cfg.darts_temp_proportion = proportion;
  n->cfg.bn_temp_proportion = proportion;
  return TDNNF_OK;
}

int tdnnf_net_set_batchnorm_sync(tdnnf_net *n, TDNNF_ALLREDUCE_FN *allreduce, void *ctx, int world_size) {
  TDNNF_REQUIRE(n && world_size >= 1, "net_set_batchnorm_sync: bad arguments");
  n->bn_sync.fn = allreduce;
  n->bn_sync.ctx = ctx;
  n->bn_sync.world = world_size;
  return TDNNF_OK;
}

int tdnnf_net_set_learning_rate_factor(tdnnf_net *n, const char *name_pattern, float factor, int *num_set) {
  TDNNF_REQUIRE(n && name_pattern && factor >= 0.f, "net_set_learning_rate_factor: bad arguments (the factor must be >= 0)");
  int cnt = 0;
  for (auto &cd : n->comps)
    if (cd.updatable && name_matches(cd.name.c_str(), name_pattern)) {
      cd.lr_factor = factor;
      cnt++;
    }
  if (num_set) *num_set = cnt;
  return TDNNF_OK;
}

int tdnnf_net_component_num_alpha(const tdnnf_net *n, int i) {
  return n && i >= 0 && i < (int)n->comps.size() ? n->comps[i].num_alpha : 0;
}
int tdnnf_net_num_random_draws(const tdnnf_net *n) { return n ? n->num_draws : 0; }
int tdnnf_net_set_random_draws(tdnnf_net *n, const float *draws) {
  TDNNF_REQUIRE(n && (draws || n->num_draws == 0), "net_set_random_draws: null argument");
  n->draws = draws;
  return TDNNF_OK;
}

int tdnnf_net_input_frames(const tdnnf_net *n, int *num_t_in, int *first_t) {
  TDNNF_REQUIRE(n, "net_input_frames: null net");
  if (num_t_in) *num_t_in = n->g_feat.n;
  if (first_t) *first_t = n->g_feat.t0;
  return TDNNF_OK;
}

int tdnnf_net_set_buffers(tdnnf_net *n, float *params, float *grads) {
  TDNNF_REQUIRE(n && params && grads && ((uintptr_t)params & 15) == 0 && ((uintptr_t)grads & 15) == 0,
                "net_set_buffers: buffers must be non-null and 16-byte aligned");
  n->params = params;
  n->grads = grads;
  return TDNNF_OK;
}

int tdnnf_net_num_grad_buckets(const tdnnf_net *n) { return n ? (int)n->buckets.size() : 0; }
int tdnnf_net_grad_bucket(const tdnnf_net *n, int i, long long *begin, long long *end) {
  TDNNF_REQUIRE(n && i >= 0 && i < (int)n->buckets.size(), "net_grad_bucket: bad index");
  if (begin) *begin = n->buckets[i].begin;
  if (end) *end = n->buckets[i].end;
  return TDNNF_OK;
}
int tdnnf_net_wait_grad_bucket(const tdnnf_net *n, int i, tdnnf_stream stream) {
  TDNNF_REQUIRE(n && i >= 0 && i < (int)n->buckets.size(), "net_wait_grad_bucket: bad index");
  TDNNF_HIP(hipStreamWaitEvent((hipStream_t)stream, n->buckets[i].ready, 0));
  return TDNNF_OK;
}

int tdnnf_net_set_capture(tdnnf_net *n, int on) {
  TDNNF_REQUIRE(n, "net_set_capture: null net");
  n->capture_on = on != 0;
  return TDNNF_OK;
}

int tdnnf_net_activation_dims(const tdnnf_net *n, const char *name, int *rows, int *cols) {
  TDNNF_REQUIRE(n && name, "net_activation_dims: null argument");
  for (auto &kv : n->named)
    if (kv.first == name) {
      if (rows) *rows = kv.second.rows;
      if (cols) *cols = kv.second.cols;
      return TDNNF_OK;
    }
  set_error("net_activation_dims: unknown activation '%s'", name);
  return TDNNF_EINVAL;
}

int tdnnf_net_get_activation(const tdnnf_net *n, const char *name, tdnnf_mat *out, tdnnf_stream stream) {
  TDNNF_REQUIRE(n && name && mat_ok(out), "net_get_activation: bad argument");
  for (auto &kv : n->named)
    if (kv.first == name) {
      TDNNF_REQUIRE(out->rows == kv.second.rows && out->cols == kv.second.cols, "net_get_activation: %s is %d x %d", name,
                    kv.second.rows, kv.second.cols);
      return tdnnf_sum_scaled(&kv.second, 1.0f, nullptr, 0.f, out, stream);
    }
  set_error("net_get_activation: unknown activation '%s'", name);
  return TDNNF_EINVAL;
}

}  // extern "C"
