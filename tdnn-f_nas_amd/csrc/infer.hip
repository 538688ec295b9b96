// infer.hip -- forward-only inference of a trained model over whole utterances (tdnnf_infer_*, include/tdnnf_hip.h "inference").
//
// nnet3's DecodableNnetSimple (UPSTREAM, not shipped) restated for the TDNN-F graphs of net_graph.hip: utterances are cut into chunks of
// F input frames, a batch of up to max_chunks chunks runs the network once, and the output rows that lie inside their utterance
// go straight to the caller's stacked output.  The schedule is written once for this pass, the f16x3 pass and the streaming one
// (infer_forward.hip); this file keeps the entries, the chunk plan, a batch's input and the description of its buffers.  Memory: two ping-pong activation buffers (a layer's input
// dies once its bypass is consumed), the linear and head temporaries and the chunk table; no gradients, natural-gradient
// state, chain workspace or side streams.  Everything runs on the caller's stream.  An object made by tdnnf_infer_create_arith with
// gemm_precision 3 runs the same schedule from f16 planes: infer_planes.hip (the object itself: infer_state.h).
#include <string.h>

#include <vector>

#include "common.h"
#include "infer_forward.h"
#include "infer_state.h"
#include "net_model.h"

using namespace tdnnf;

namespace {

constexpr int kTab = 6;  // device chunk table: [first feature row of the utterance, T_u, k F, stacked i-vector row, first output row, n_k]

// Spliced LDA input of a batch of B chunks, t-major (row k B + b, k < nk): [feats(t_k), feats(t_k + 1), feats(t_k + 2) ; i-vector]
// with t_k = kF + first_t + k clamped to the utterance -- the layout tdnnf_splice_input produces, read through the chunk table.
// VEC 4: 16-byte loads and stores (feat_dim, ivector_dim, strides and pointers multiples of 4 floats).
template <int VEC>
__global__ __launch_bounds__(256) void infer_gather_kernel(MatView feats, MatView iv, const int *tab, int B, int nk, int first_t, MatView out) {
  const int fd = feats.cols, cv = out.cols / VEC;
  const long long total = (long long)out.rows * cv;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int r = (int)(e / cv), c = (int)(e % cv) * VEC, k = r / B, b = r % B;
    const int *ch = tab + kTab * b;
    const float *src;
    if (c < 3 * fd) {
      int t = ch[2] + first_t + k + c / fd;
      t = t < 0 ? 0 : (t >= ch[1] ? ch[1] - 1 : t);
      src = feats.data + (size_t)(ch[0] + t) * feats.stride + c % fd;
    } else {
      src = iv.data + (size_t)ch[3] * iv.stride + (c - 3 * fd);
    }
    float *dst = out.data + (size_t)r * out.stride + c;
    if (VEC == 4) *reinterpret_cast<float4 *>(dst) = *reinterpret_cast<const float4 *>(src);
    else *dst = *src;
  }
}

// row_map[j B + b] = first output row of chunk b + j for the chunk's valid rows j < n_k, -1 past the end of its utterance
__global__ void infer_row_map_kernel(const int *tab, int B, int Tout, int *row_map) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= B * Tout) return;
  const int j = m / B, b = m % B;
  row_map[m] = j < tab[kTab * b + 5] ? tab[kTab * b + 4] + j : -1;
}

}  // namespace

namespace tdnnf {

int infer_batch_input(tdnnf_infer *q, const tdnnf_mat *feats, const tdnnf_mat *iv, const int *tab, int B, hipStream_t s) {
  const tdnnf_net_config &c = q->model->cfg;
  const int lda_dim = 3 * c.feat_dim + c.ivector_dim, N0 = q->g_lda.n * B, No = q->Tout * B;
  tdnnf_mat lda_in = M(q->lda_in, N0, lda_dim);
  const MatView fv = view(feats), ivv = view(iv), ov = view(&lda_in);
  const bool v4 = vec4_ok(fv) && vec4_ok(ivv) && vec4_ok(ov);
  const long long work = (long long)N0 * lda_dim / (v4 ? 4 : 1);
  if (v4) hipLaunchKernelGGL(infer_gather_kernel<4>, dim3(grid_for(work, 256)), dim3(256), 0, s, fv, ivv, tab, B, q->g_lda.n, q->g_feat.t0, ov);
  else hipLaunchKernelGGL(infer_gather_kernel<1>, dim3(grid_for(work, 256)), dim3(256), 0, s, fv, ivv, tab, B, q->g_lda.n, q->g_feat.t0, ov);
  TDNNF_LAUNCH_CHECK();
  hipLaunchKernelGGL(infer_row_map_kernel, dim3((No + 255) / 256), dim3(256), 0, s, tab, B, q->Tout, q->head.row_map);
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

// Where a batch of B chunks lives: two ping-pong activation buffers (a layer's input dies once its bypass is consumed), the linear and
// head temporaries.  The buffers are the object's, so the description changes with B alone and is kept from one batch to the next.
const FwdBuffers &infer_buffers(tdnnf_infer *q, int B) {
  FwdBuffers &b = q->fwd;
  if (q->fwd_B == B) return b;
  const tdnnf_net_config &c = q->model->cfg;
  const int Hd = c.hidden_dim, S = c.prefinal_small_dim, P = c.num_pdfs, lda_dim = 3 * c.feat_dim + c.ivector_dim;
  const int N0 = q->g_lda.n * B, No = q->Tout * B;
  b.lda_in = M(q->lda_in, N0, lda_dim);
  b.lda_out = M(q->lda_out, N0, lda_dim);
  b.x0 = M(q->act[0], N0, Hd);
  int cur = 0;
  for (size_t l = 0; l < q->layers.size(); l++, cur ^= 1) {
    const TdnnfLayer &L = q->layers[l];
    FwdLayer &f = b.layers[l];
    layer_tdnns(q->model, (int)l, L.gin, L.glin, L.glin, L.gout, B, &f.lin, &f.aff);
    f.lin_in = M(q->act[cur], L.gin.n * B, Hd);
    f.lin_out = M(q->lin, f.lin.rows_out, L.bn);
    f.perm_out = f.aff_in = L.perm ? M(q->lin_perm, f.lin.rows_out, L.bn) : f.lin_out;
    f.byp = sub_grid_view(q->act[cur], L.gin, L.gout, B, Hd);
    f.out = M(q->act[cur ^ 1], f.aff.rows_out, Hd);
    f.relu = L.gout.step != L.gin.step ? M(q->relu_tmp, f.aff.rows_out, Hd) : tdnnf_mat{nullptr, 0, 0, 0};
    f.out_times = L.gout.n;
  }
  b.top = M(q->act[cur], No, Hd);
  b.pl = M(q->head.pl, No, S);
  b.b1 = M(q->act[cur ^ 1], No, Hd);
  b.b2 = M(q->head.b2, No, S);
  b.y = M(q->head.y, No, P);
  b.lsm = M(q->head.lsm, No, P);
  b.row_map = q->head.row_map;
  q->fwd_B = B;
  return b;
}

}  // namespace tdnnf

namespace {

void layout(tdnnf_infer *q, Arena &A) {
  const tdnnf_net_config &c = q->model->cfg;
  const int B = q->max_chunks, Hd = c.hidden_dim, lda_dim = 3 * c.feat_dim + c.ivector_dim;
  const long long N0 = (long long)q->g_lda.n * B, No = (long long)q->Tout * B;
  long long rows = std::max(N0, No), lin_rows = 0, relu_rows = 0;
  int bn_max = 0;
  bool perm = false;
  for (auto &L : q->layers) {
    rows = std::max(rows, (long long)std::max(L.gin.n, L.gout.n) * B);
    lin_rows = std::max(lin_rows, (long long)L.glin.n * B);
    bn_max = std::max(bn_max, L.bn);
    perm = perm || L.perm;
    if (L.gout.step != L.gin.step) relu_rows = std::max(relu_rows, (long long)L.gout.n * B);
  }
  q->lda_in = A.mat(N0, lda_dim);
  q->lda_out = A.mat(N0, lda_dim);
  q->act[0] = A.mat(rows, Hd);
  q->act[1] = A.mat(rows, Hd);
  q->lin = A.mat(lin_rows, bn_max);
  q->lin_perm = perm ? A.mat(lin_rows, bn_max) : nullptr;
  q->relu_tmp = relu_rows ? A.mat(relu_rows, Hd) : nullptr;
  infer_head_layout(c, q->which, q->nbn, No, false, 0, A, &q->head);
}

// chunk plan of section "inference" in tdnnf_hip.h: per chunk (utterance, k F, i-vector row within the utterance, n_k)
int make_plan(int F, int fsf, int num_utts, const int *frames, const int *iv_rows, int period, std::vector<int> &plan) {
  TDNNF_REQUIRE(fsf >= 1 && F > 0 && F % fsf == 0, "infer: frames_per_chunk %d must be a positive multiple of frame_subsampling %d", F, fsf);
  TDNNF_REQUIRE(num_utts >= 0 && (num_utts == 0 || frames), "infer: frames_host must hold num_utts lengths");
  TDNNF_REQUIRE(period <= 0 || num_utts == 0 || iv_rows, "infer: ivector_period > 0 needs ivector_rows_host");
  plan.clear();
  const int Tout = F / fsf;
  for (int u = 0; u < num_utts; u++) {
    TDNNF_REQUIRE(frames[u] >= 0, "infer: utterance %d has %d frames", u, frames[u]);
    const int R = period > 0 ? iv_rows[u] : 1;
    TDNNF_REQUIRE(R >= 1, "infer: utterance %d has no i-vector rows", u);
    const int O = (frames[u] + fsf - 1) / fsf;
    for (int k = 0; k * Tout < O; k++) {
      const int n = std::min(Tout, O - k * Tout);
      int row = 0;
      if (period > 0) row = std::min((int)(((long long)(k * F / fsf) + n / 2) * fsf / period), R - 1);
      plan.insert(plan.end(), {u, k * F, row, n});
    }
  }
  return TDNNF_OK;
}

// one batch of B chunks whose input and row map are in place: the one schedule, on the f32 GEMM or from the f16 planes
int forward_batch(tdnnf_infer *q, int B, tdnnf_mat *out, hipStream_t s, bool count) {
  FwdCounts cnt;
  if (q->planes) {
    CK(infer_planes_forward(q, B, out, s, &cnt));
  } else {
    CK(infer_forward(q->model, q->head.coef, q->which, B, infer_buffers(q, B), out, infer_gemm_f32, const_cast<tdnnf_net *>(q->model), s, &cnt));
    q->f32_gemms += cnt.gemms;  // lda, tdnn1, two per layer, prefinal-l, the head's three
  }
  if (count) {
    q->fused = cnt.fused;
    q->fallback = cnt.fallback;
  }
  return TDNNF_OK;
}

// the object behind both create entries (`who`): the checks, grids, BatchNorm table, arena; gemm_precision 3: the plane buffers as well.
// own_arith: the model's own cfg.gemm_precision is the trainer's arithmetic, this object reads the f32 parameters and statistics only
int create_object(const char *who, const tdnnf_net *model, int frames_per_chunk, int max_chunks, int which_output, int gemm_precision, bool own_arith,
                  tdnnf_infer **out) {
  TDNNF_REQUIRE(max_chunks >= 1 && which_output >= 0 && which_output <= 1, "%s: max_chunks must be >= 1, which_output 0 or 1", who);
  TDNNF_REQUIRE(model && out, "%s: null argument", who);
  tdnnf_net_config c = model->cfg;
  if (own_arith) c.gemm_precision = 0;
  CK(infer_check_model(c, frames_per_chunk, who, "frames_per_chunk"));
  tdnnf_infer *q = new tdnnf_infer();
  q->model = model;
  q->F = frames_per_chunk;
  q->fsf = c.frame_subsampling;
  q->Tout = frames_per_chunk / c.frame_subsampling;
  q->max_chunks = max_chunks;
  q->which = which_output;
  q->fwd.layers.resize(c.num_layers);
  int rc = net_layer_grids(c, q->Tout, q->layers, &q->g_lda);
  if (rc == TDNNF_OK && q->g_lda.step != 1) {
    set_error("infer_create: the first tdnnf layers must run at the input frame rate");
    rc = TDNNF_EINVAL;
  }
  if (rc != TDNNF_OK) {
    delete q;
    return rc;
  }
  q->g_feat = feat_grid(q->g_lda);
  // BatchNorm stages: tdnn1, the tdnnf layers, the chosen head's two (the model's statistics, by reference)
  q->nbn = infer_bn_table(model, which_output, &q->bn);
  Arena sizing;
  layout(q, sizing);
  if (hipMalloc((void **)&q->arena, sizing.off + 1024) != hipSuccess) {
    (void)hipGetLastError();
    set_error("infer_create: cannot allocate %zu bytes of activations", sizing.off + 1024);
    delete q;
    return TDNNF_EHIP;
  }
  Arena real;
  real.base = q->arena;
  layout(q, real);
  if (gemm_precision == 3) {
    rc = infer_planes_create(q);
    if (rc != TDNNF_OK) {
      tdnnf_infer_destroy(q);
      return rc;
    }
  }
  *out = q;
  return TDNNF_OK;
}

}  // namespace

extern "C" {

int tdnnf_infer_create(const tdnnf_net *model, int frames_per_chunk, int max_chunks, int which_output, tdnnf_infer **out) {
  return create_object("infer_create", model, frames_per_chunk, max_chunks, which_output, 0, false, out);
}

int tdnnf_infer_create_arith(const tdnnf_net *model, int frames_per_chunk, int max_chunks, int which_output, int gemm_precision, tdnnf_infer **out) {
  TDNNF_REQUIRE(gemm_precision == 0 || gemm_precision == 3,
                "infer_create_arith: gemm_precision %d: inference runs exact f32 (gemm_precision 0) or f16x3 (gemm_precision 3)", gemm_precision);
  return create_object("infer_create_arith", model, frames_per_chunk, max_chunks, which_output, gemm_precision, true, out);
}

void tdnnf_infer_destroy(tdnnf_infer *q) {
  if (!q) return;
  infer_planes_destroy(q->planes);
  hipFree(q->arena);
  hipFree(q->table);
  delete q;
}

int tdnnf_chunk_plan(int frames_per_chunk, int frame_subsampling, int num_utts, const int *frames_host, const int *ivector_rows_host,
                     int ivector_period, int *chunks_out, int capacity, int *num_chunks) {
  TDNNF_REQUIRE(num_chunks && capacity >= 0 && (chunks_out || capacity == 0), "chunk_plan: bad arguments");
  std::vector<int> plan;
  CK(make_plan(frames_per_chunk, frame_subsampling, num_utts, frames_host, ivector_rows_host, ivector_period, plan));
  const int nch = (int)(plan.size() / 4);
  *num_chunks = nch;
  if (capacity > 0) memcpy(chunks_out, plan.data(), sizeof(int) * 4 * std::min(nch, capacity));
  TDNNF_REQUIRE(nch <= capacity, "chunk_plan: %d chunks, capacity %d", nch, capacity);
  return TDNNF_OK;
}

int tdnnf_infer_plan(const tdnnf_infer *q, int num_utts, const int *frames_host, const int *ivector_rows_host, int ivector_period,
                     int *chunks_out, int capacity, int *num_chunks) {
  TDNNF_REQUIRE(q, "infer_plan: null argument");
  return tdnnf_chunk_plan(q->F, q->fsf, num_utts, frames_host, ivector_rows_host, ivector_period, chunks_out, capacity, num_chunks);
}

int tdnnf_infer_compute(tdnnf_infer *q, int num_utts, const int *frames_host, const tdnnf_mat *feats, const int *ivector_rows_host,
                        const tdnnf_mat *ivectors, int ivector_period, tdnnf_mat *out, tdnnf_stream stream) {
  TDNNF_REQUIRE(q && mat_ok(feats) && mat_ok(ivectors) && mat_ok(out), "infer_compute: bad arguments");
  const tdnnf_net *n = q->model;
  TDNNF_REQUIRE(n->params, "infer_compute: the model net has no parameter buffer (net_set_buffers)");
  const tdnnf_net_config &c = n->cfg;
  std::vector<int> plan;
  CK(make_plan(q->F, q->fsf, num_utts, frames_host, ivector_rows_host, ivector_period, plan));
  long long sumT = 0, sumR = 0, sumO = 0;
  std::vector<long long> feat0(num_utts), iv0(num_utts), out0(num_utts);
  for (int u = 0; u < num_utts; u++) {
    feat0[u] = sumT;
    iv0[u] = sumR;
    out0[u] = sumO;
    sumT += frames_host[u];
    sumR += ivector_period > 0 ? ivector_rows_host[u] : 1;
    sumO += (frames_host[u] + q->fsf - 1) / q->fsf;
  }
  TDNNF_REQUIRE(feats->rows == sumT && feats->cols == c.feat_dim, "infer_compute: feats must be %lld x %d (the utterances stacked)", sumT, c.feat_dim);
  TDNNF_REQUIRE(ivectors->rows == sumR && ivectors->cols == c.ivector_dim, "infer_compute: ivectors must be %lld x %d", sumR, c.ivector_dim);
  TDNNF_REQUIRE(out->rows == sumO && out->cols == c.num_pdfs, "infer_compute: out must be %lld x %d", sumO, c.num_pdfs);
  TDNNF_REQUIRE(sumT < (1LL << 31) && sumR < (1LL << 31), "infer_compute: too many rows");
  const int nch = (int)(plan.size() / 4);
  q->fused = q->fallback = 0;
  q->plane_gemms = q->f32_gemms = 0;
  if (nch == 0) return TDNNF_OK;
  hipStream_t s = (hipStream_t)stream;
  // ---- the chunk table of the whole call, uploaded once
  q->host_table.resize((size_t)kTab * nch);
  for (int k = 0; k < nch; k++) {
    const int *p = &plan[4 * k];
    int *t = &q->host_table[(size_t)kTab * k];
    const int u = p[0];
    t[0] = (int)feat0[u];
    t[1] = frames_host[u];
    t[2] = p[1];
    t[3] = (int)iv0[u] + p[2];
    t[4] = (int)out0[u] + (p[1] / q->fsf);
    t[5] = p[3];
  }
  if (q->table_cap < q->host_table.size()) {
    TDNNF_HIP(hipStreamSynchronize(s));  // (the previous call's batches may still read the old table)
    hipFree(q->table);
    q->table = nullptr;
    q->table_cap = 0;
    TDNNF_HIP(hipMalloc((void **)&q->table, sizeof(int) * q->host_table.size()));
    q->table_cap = q->host_table.size();
  }
  TDNNF_HIP(hipMemcpyAsync(q->table, q->host_table.data(), sizeof(int) * q->host_table.size(), hipMemcpyHostToDevice, s));
  // ---- the model's BatchNorm statistics as test-mode scale / offset (read at every call)
  TDNNF_HIP(infer_bn_coef(q->bn, q->nbn, q->head.coef, s));
  if (q->planes) CK(infer_planes_begin(q, s));  // ... and its weights as f16 planes
  for (int k0 = 0; k0 < nch; k0 += q->max_chunks) {
    const int B = std::min(q->max_chunks, nch - k0);
    const int *tab = q->table + (size_t)kTab * k0;
    CK(infer_batch_input(q, feats, ivectors, tab, B, s));  // clamped chunk windows + i-vector, spliced for the lda layer in one pass
    CK(forward_batch(q, B, out, s, k0 == 0));
  }
  return TDNNF_OK;
}

int tdnnf_infer_counts(const tdnnf_infer *q, int *fused_layers, int *fallback_passes) {
  TDNNF_REQUIRE(q, "infer_counts: null argument");
  if (fused_layers) *fused_layers = q->fused;
  if (fallback_passes) *fallback_passes = q->fallback;
  return TDNNF_OK;
}

int tdnnf_infer_gemm_counts(const tdnnf_infer *q, long long *plane_gemms, long long *f32_gemms) {
  TDNNF_REQUIRE(q, "infer_gemm_counts: null argument");
  if (plane_gemms) *plane_gemms = q->plane_gemms;
  if (f32_gemms) *f32_gemms = q->f32_gemms;
  return TDNNF_OK;
}

}  // extern "C"
