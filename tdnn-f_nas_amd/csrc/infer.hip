// infer.hip -- forward-only inference of a trained model over whole utterances (tdnnf_infer_*, include/tdnnf_hip.h "inference").
//
// nnet3's DecodableNnetSimple (UPSTREAM, not shipped) restated for the TDNN-F graphs of net_graph.hip: utterances are cut into chunks of
// F input frames, a batch of up to max_chunks chunks runs the network once, and the output rows that lie inside their utterance
// go straight to the caller's stacked output.  The schedule is the trainer's forward pass (net_step.hip) in test mode (cv_update) without the
// separate elementwise passes: every BatchNorm -- and a TDNN-F layer's bypass -- is applied while the GEMM stores its tile
// (RowsGemmArgs::col_scale / col_offset / post_add, gemm_f32.h).  Memory: two ping-pong activation buffers (a layer's input
// dies once its bypass is consumed), the linear and head temporaries and the chunk table; no gradients, natural-gradient
// state, chain workspace or side streams.  Everything runs on the caller's stream.  An object made by tdnnf_infer_create_arith with
// gemm_precision 3 runs the same schedule from f16 planes: infer_planes.hip (the object itself: infer_state.h).
#include <math.h>
#include <string.h>

#include <vector>

#include "common.h"
#include "fused.h"
#include "gemm_f32.h"
#include "infer_parts.h"
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

// infer_scatter_rows: out[row_map[m]] = in[m] for the rows that have one (the log-softmax of the xent head)
template <int VEC>
__global__ __launch_bounds__(256) void infer_scatter_kernel(MatView in, const int *row_map, MatView out) {
  const int cv = in.cols / VEC;
  const long long total = (long long)in.rows * cv;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int m = (int)(e / cv), c = (int)(e % cv) * VEC, mo = row_map[m];
    if (mo < 0) continue;
    if (VEC == 4) *reinterpret_cast<float4 *>(out.data + (size_t)mo * out.stride + c) = *reinterpret_cast<const float4 *>(in.data + (size_t)m * in.stride + c);
    else out.data[(size_t)mo * out.stride + c] = in.data[(size_t)m * in.stride + c];
  }
}

// infer_bn_coef (infer_parts.h): the arithmetic of bn_test_memo_kernel (BatchNormComponent::ComputeDerived,
// nnet-normalize-component.cc:682-715).
__global__ void infer_bn_coef_kernel(BnTable tb, float *coef) {
  const int i = blockIdx.y, D = tb.D[i], d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= D) return;
  const double *stats = tb.stats[i];
  float *c = coef + tb.coef_off[i];
  const double count = stats[0];
  const float off = (float)(stats[1 + d] * (-1.0 / count));
  float sc = (float)(stats[1 + D + d] * (1.0 / count));
  sc += -1.0f * off * off;
  c[D + d] = sc;
  sc = floor_keep_nan(sc, 0.f) + 1.0e-3f;
  sc = 1.0f / sqrtf(sc);
  c[d] = -off;
  c[2 * D + d] = sc;
  c[3 * D + d] = off * sc;
}

}  // namespace

namespace tdnnf {

int infer_check_model(const tdnnf_net_config &c, int frames, const char *who, const char *frames_name) {
  TDNNF_REQUIRE(c.darts_num_offsets < 2, "%s: the offset supernet (darts_num_offsets = %d) is not supported: derive a child first", who,
                c.darts_num_offsets);
  TDNNF_REQUIRE(c.bn_num_choices == 0, "%s: the bottleneck supernet (bn_num_choices = %d) is not supported: derive a child first", who,
                c.bn_num_choices);
  TDNNF_REQUIRE(c.gemm_precision == 0, "%s: gemm_precision %d: inference runs exact f32 only (gemm_precision 0)", who, c.gemm_precision);
  TDNNF_REQUIRE(frames > 0 && frames % c.frame_subsampling == 0, "%s: %s %d must be a positive multiple of frame_subsampling %d", who, frames_name,
                frames, c.frame_subsampling);
  return TDNNF_OK;
}

int infer_bn_table(const tdnnf_net *model, int which_output, BnTable *bn) {
  memset(bn, 0, sizeof(*bn));
  const long long bstride = infer_bn_stride(model->cfg);
  int nbn = 0;
  for (const StatBlock &b : stat_blocks(model)) {
    if (b.relu || (b.head >= 0 && b.head != which_output)) continue;
    bn->stats[nbn] = b.p();
    bn->D[nbn] = b.D;
    bn->coef_off[nbn] = nbn * bstride;
    nbn++;
  }
  return nbn;
}

hipError_t infer_bn_coef(const BnTable &bn, int nbn, float *coef, hipStream_t s) {
  int dmax = 0;
  for (int i = 0; i < nbn; i++) dmax = std::max(dmax, bn.D[i]);
  hipLaunchKernelGGL(infer_bn_coef_kernel, dim3((dmax + 255) / 256, nbn), dim3(256), 0, s, bn, coef);
  return hipGetLastError();
}

hipError_t infer_scatter_rows(const MatView &in, const int *row_map, const MatView &out, hipStream_t s) {
  const bool v4 = vec4_ok(in) && vec4_ok(out);
  const long long work = (long long)in.rows * in.cols / (v4 ? 4 : 1);
  if (v4) hipLaunchKernelGGL(infer_scatter_kernel<4>, dim3(grid_for(work, 256)), dim3(256), 0, s, in, row_map, out);
  else hipLaunchKernelGGL(infer_scatter_kernel<1>, dim3(grid_for(work, 256)), dim3(256), 0, s, in, row_map, out);
  return hipGetLastError();
}

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
  hipLaunchKernelGGL(infer_row_map_kernel, dim3((No + 255) / 256), dim3(256), 0, s, tab, B, q->Tout, q->row_map);
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

// rows GEMM of one TdnnComponent (or affine: ix = one tap) with the inference epilogue
int gemm_post(const tdnnf_tdnn_indexes &ix, const tdnnf_mat &in, const float *W, int ldw, int Do, int Di, const float *bias, int relu,
              const float *coef, const tdnnf_mat *add, float add_scale, const int *row_map, const tdnnf_mat &out, hipStream_t s) {
  RowsGemmArgs a;
  memset(&a, 0, sizeof(a));
  a.A = in.data;
  a.lda = (long long)in.stride * ix.row_stride;
  a.B = W;
  a.ldb = ldw;
  a.C = out.data;
  a.ldc = out.stride;
  a.M = out.rows;
  a.N = Do;
  a.bias = bias;
  a.init_mode = bias ? 1 : 2;
  a.relu = relu;
  a.nseg = ix.num_offsets;
  for (int i = 0; i < a.nseg; i++) {
    a.seg[i].a_off = (long long)ix.row_offsets[i] * in.stride;
    a.seg[i].b_off = (long long)i * Di;
    a.seg[i].klen = Di;
    a.seg[i].m_lo = 0;
    a.seg[i].m_hi = a.M;
  }
  if (coef) {  // [mean | variance | scale | offset]
    a.col_scale = coef + 2 * Do;
    a.col_offset = coef + 3 * Do;
  }
  if (add) {
    a.add = add->data;
    a.ldadd = add->stride;
    a.add_scale = add_scale;
    a.add_lo = 0;
    a.add_hi = a.M;
    a.post_add = 1;
  }
  a.row_map = row_map;
  TDNNF_HIP(rows_gemm(a, true, s));
  return TDNNF_OK;
}

}  // namespace tdnnf

namespace {

void layout(tdnnf_infer *q, Arena &A) {
  const tdnnf_net_config &c = q->model->cfg;
  const int B = q->max_chunks, Hd = c.hidden_dim, S = c.prefinal_small_dim, P = c.num_pdfs, lda_dim = 3 * c.feat_dim + c.ivector_dim;
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
  q->pl = A.mat(No, S);
  q->b2 = A.mat(No, S);
  q->y = q->which == 1 ? A.mat(No, P) : nullptr;
  q->lsm = q->which == 1 ? A.mat(No, P) : nullptr;
  q->row_map = A.take<int>((size_t)No);
  q->coef = A.take<float>((size_t)q->nbn * 4 * ldpad(std::max(Hd, S)));
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

// one batch of B chunks (their table entries at tab)
int forward_batch(tdnnf_infer *q, const tdnnf_mat *feats, const tdnnf_mat *iv, const int *tab, int B, tdnnf_mat *out, hipStream_t s, bool count) {
  const tdnnf_net *n = q->model;
  const tdnnf_net_config &c = n->cfg;
  const int Hd = c.hidden_dim, S = c.prefinal_small_dim, P = c.num_pdfs, lda_dim = 3 * c.feat_dim + c.ivector_dim, Tout = q->Tout;
  const int N0 = q->g_lda.n * B, No = Tout * B;
  const long long bstride = 4LL * ldpad(std::max(Hd, S));
  auto coef = [&](int i) { return q->coef + i * bstride; };
  auto W = [&](int comp) { return net_W(n, comp); };
  auto bias = [&](int comp) { return net_bias(n, comp); };
  // ---- input: clamped chunk windows + i-vector, spliced for the lda layer in one pass
  CK(infer_batch_input(q, feats, iv, tab, B, s));
  tdnnf_mat lda_in = M(q->lda_in, N0, lda_dim), lda_out = M(q->lda_out, N0, lda_dim);
  CK(tdnnf_affine_propagate(&lda_in, W(n->c_lda), lda_dim, bias(n->c_lda), lda_dim, &lda_out, s));
  tdnnf_tdnn_indexes ix1;
  memset(&ix1, 0, sizeof(ix1));
  ix1.row_stride = 1;
  ix1.num_offsets = 1;
  // ---- tdnn1: affine + ReLU + BatchNorm in one GEMM
  int cur = 0;
  CK(gemm_post(ix1, lda_out, W(n->tdnn1.comp), lda_dim, Hd, lda_dim, bias(n->tdnn1.comp), 1, coef(0), nullptr, 0.f, nullptr, M(q->act[0], N0, Hd), s));
  int fused = 1, fallback = 0;
  for (size_t l = 0; l < q->layers.size(); l++) {
    const TdnnfLayer &L = q->layers[l];
    const TdnnfLayer &ML = n->layers[l];  // component ids, taps
    std::vector<int> lin_off, aff_off;
    layer_taps(c, L, &lin_off, &aff_off);
    Tdnn lin, aff;
    make_tdnn(&lin, ML.lin.comp, Hd, L.bn, lin_off, L.gin, L.glin, B);
    make_tdnn(&aff, ML.aff.comp, L.bn, Hd, aff_off, L.glin, L.gout, B);
    tdnnf_mat in = M(q->act[cur], L.gin.n * B, Hd), lo = M(q->lin, lin.rows_out, L.bn);
    CK(tdnn_propagate_impl(&lin.ix, &in, W(lin.comp), lin.K * Hd, L.bn, Hd, nullptr, nullptr, 2, 0, &lo, s));
    tdnnf_mat aff_in = lo;
    if (L.perm) {
      aff_in = M(q->lin_perm, lin.rows_out, L.bn);
      CK(tdnnf_reorder_rows(&lo, B, aff.ix.row_stride, 1, &aff_in, s));
    }
    tdnnf_mat byp = sub_grid_view(q->act[cur], L.gin, L.gout, B, Hd), o = M(q->act[cur ^ 1], aff.rows_out, Hd);
    if (L.gout.step == L.gin.step) {  // noop = Sum(Scale(bypass, input rows), batchnorm(relu(affine))) while the tile is stored
      CK(gemm_post(aff.ix, aff_in, W(aff.comp), aff.K * L.bn, Hd, L.bn, bias(aff.comp), 1, coef(1 + (int)l), &byp, c.bypass_scale, nullptr, o, s));
      fused++;
    } else {  // bypass rows strided against the output rows: ReLU in the GEMM, BatchNorm + bypass in the trainer's pass
      tdnnf_mat r = M(q->relu_tmp, aff.rows_out, Hd);
      CK(tdnn_propagate_impl(&aff.ix, &aff_in, W(aff.comp), aff.K * L.bn, Hd, L.bn, bias(aff.comp), nullptr, 1, 1, &r, s));
      const tdnnf_mat x{q->relu_tmp, L.gout.n, byp.cols, B * ldpad(Hd)}, ov{q->act[cur ^ 1], L.gout.n, byp.cols, B * ldpad(Hd)};
      TDNNF_HIP(bn_apply_bypass(view(&x), coef(1 + (int)l), Hd, ldpad(Hd), view(&byp), c.bypass_scale, view(&ov), s, nullptr, B));
      fallback++;
    }
    cur ^= 1;
  }
  // ---- the chosen head: prefinal-l, affine + ReLU + batchnorm1, linear + batchnorm2, output
  const auto &H = n->head[q->which];
  const int nb = (int)q->layers.size() + 1;
  tdnnf_mat top = M(q->act[cur], No, Hd), pl = M(q->pl, No, S), b1 = M(q->act[cur ^ 1], No, Hd), b2 = M(q->b2, No, S);
  CK(tdnnf_affine_propagate(&top, W(n->c_prefinal_l), Hd, nullptr, S, &pl, s));
  CK(gemm_post(ix1, pl, W(H.c_affine), S, Hd, S, bias(H.c_affine), 1, coef(nb), nullptr, 0.f, nullptr, b1, s));
  CK(gemm_post(ix1, b1, W(H.c_linear), Hd, S, Hd, nullptr, 0, coef(nb + 1), nullptr, 0.f, nullptr, b2, s));
  fused += 2;
  if (q->which == 0) {  // rows inside their utterance straight into the caller's output
    tdnnf_mat ym = *out;
    ym.rows = No;
    CK(gemm_post(ix1, b2, W(H.c_output), S, P, S, bias(H.c_output), 0, nullptr, nullptr, 0.f, q->row_map, ym, s));
  } else {
    tdnnf_mat y = M(q->y, No, P), lsm = M(q->lsm, No, P);
    CK(tdnnf_affine_propagate(&b2, W(H.c_output), S, bias(H.c_output), P, &y, s));
    CK(tdnnf_log_softmax_propagate(&y, &lsm, s));
    TDNNF_HIP(infer_scatter_rows(view(&lsm), q->row_map, view(out), s));
  }
  if (count) {
    q->fused = fused;
    q->fallback = fallback;
  }
  q->f32_gemms += 2 * (long long)q->layers.size() + 6;  // lda, tdnn1, two per layer, prefinal-l, the head's three
  return TDNNF_OK;
}

// the object behind both create entries (the model is checked): grids, BatchNorm table, arena; gemm_precision 3: the plane buffers as well
int create_object(const tdnnf_net *model, int frames_per_chunk, int max_chunks, int which_output, int gemm_precision, tdnnf_infer **out) {
  const tdnnf_net_config &c = model->cfg;
  TDNNF_REQUIRE(max_chunks >= 1 && which_output >= 0 && which_output <= 1, "infer_create: max_chunks must be >= 1, which_output 0 or 1");
  tdnnf_infer *q = new tdnnf_infer();
  q->model = model;
  q->F = frames_per_chunk;
  q->fsf = c.frame_subsampling;
  q->Tout = frames_per_chunk / c.frame_subsampling;
  q->max_chunks = max_chunks;
  q->which = which_output;
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
  TDNNF_REQUIRE(model && out, "infer_create: null argument");
  CK(infer_check_model(model->cfg, frames_per_chunk, "infer_create", "frames_per_chunk"));
  return create_object(model, frames_per_chunk, max_chunks, which_output, 0, out);
}

int tdnnf_infer_create_arith(const tdnnf_net *model, int frames_per_chunk, int max_chunks, int which_output, int gemm_precision, tdnnf_infer **out) {
  TDNNF_REQUIRE(gemm_precision == 0 || gemm_precision == 3,
                "infer_create_arith: gemm_precision %d: inference runs exact f32 (gemm_precision 0) or f16x3 (gemm_precision 3)", gemm_precision);
  TDNNF_REQUIRE(max_chunks >= 1 && which_output >= 0 && which_output <= 1, "infer_create_arith: max_chunks must be >= 1, which_output 0 or 1");
  TDNNF_REQUIRE(model && out, "infer_create_arith: null argument");
  // the model's own cfg.gemm_precision is the trainer's arithmetic: this object reads the f32 parameters and statistics only
  tdnnf_net_config c = model->cfg;
  c.gemm_precision = 0;
  CK(infer_check_model(c, frames_per_chunk, "infer_create_arith", "frames_per_chunk"));
  return create_object(model, frames_per_chunk, max_chunks, which_output, gemm_precision, out);
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
  TDNNF_HIP(infer_bn_coef(q->bn, q->nbn, q->coef, s));
  if (q->planes) CK(infer_planes_begin(q, s));  // ... and its weights as f16 planes
  for (int k0 = 0; k0 < nch; k0 += q->max_chunks) {
    const int B = std::min(q->max_chunks, nch - k0);
    const int *tab = q->table + (size_t)kTab * k0;
    if (q->planes) {
      CK(infer_batch_input(q, feats, ivectors, tab, B, s));
      CK(infer_planes_forward(q, tab, B, out, s, k0 == 0));
    } else {
      CK(forward_batch(q, feats, ivectors, tab, B, out, s, k0 == 0));
    }
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
