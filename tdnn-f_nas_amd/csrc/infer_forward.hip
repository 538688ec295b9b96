// infer_forward.hip -- the forward-only schedule of a trained model, written once for its three readers (infer_forward.h): the trainer's
// forward pass (net_step.hip) in test mode (cv_update) without the separate elementwise passes: every BatchNorm -- and a TDNN-F layer's
// bypass -- is applied while the GEMM stores its tile (RowsGemmArgs::col_scale / col_offset / post_add, gemm_f32.h).  With it, what every
// reader needs around the schedule: the model checks, the BatchNorm coefficients, the f32 GEMM and the row-map scatter.
#include <math.h>
#include <string.h>

#include <vector>

#include "common.h"
#include "fused.h"
#include "gemm_f32.h"
#include "infer_forward.h"
#include "net_model.h"

using namespace tdnnf;

namespace {

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

// infer_bn_coef: the arithmetic of bn_test_memo_kernel (BatchNormComponent::ComputeDerived, nnet-normalize-component.cc:682-715).
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

void infer_head_layout(const tdnnf_net_config &c, int which, int nbn, long long No, bool own_b1, size_t table_ints, Arena &A, FwdHead *h) {
  const int S = c.prefinal_small_dim, P = c.num_pdfs;
  h->pl = A.mat(No, S);
  h->b1 = own_b1 ? A.mat(No, c.hidden_dim) : nullptr;
  h->b2 = A.mat(No, S);
  h->y = which == 1 ? A.mat(No, P) : nullptr;
  h->lsm = which == 1 ? A.mat(No, P) : nullptr;
  h->row_map = A.take<int>((size_t)No);
  h->table = table_ints ? A.take<int>(table_ints) : nullptr;
  h->coef = A.take<float>((size_t)nbn * infer_bn_stride(c));
}

tdnnf_tdnn_indexes one_tap() {
  tdnnf_tdnn_indexes ix;
  memset(&ix, 0, sizeof(ix));
  ix.row_stride = 1;
  ix.num_offsets = 1;
  return ix;
}

void layer_tdnns(const tdnnf_net *model, int l, const Grid &lin_in, const Grid &lin_out, const Grid &aff_in, const Grid &aff_out, int B, Tdnn *lin,
                 Tdnn *aff) {
  const tdnnf_net_config &c = model->cfg;
  const TdnnfLayer &ML = model->layers[l];  // component ids, taps, bottleneck
  std::vector<int> lin_off, aff_off;
  layer_taps(c, ML, &lin_off, &aff_off);
  make_tdnn(lin, ML.lin.comp, c.hidden_dim, ML.bn, lin_off, lin_in, lin_out, B);
  make_tdnn(aff, ML.aff.comp, ML.bn, c.hidden_dim, aff_off, aff_in, aff_out, B);
}

int gemm_post(const tdnnf_tdnn_indexes &ix, const tdnnf_mat &in, const float *W, int ldw, int Do, int Di, const float *bias, int relu,
              const float *coef, const tdnnf_mat *add, float add_scale, const int *row_map, const tdnnf_mat &out, hipStream_t s) {
  TDNNF_REQUIRE(mat_ok(&in) && mat_ok(&out) && W, "tdnn_propagate: bad matrices");
  TDNNF_REQUIRE(Do > 0 && Di > 0 && in.cols == Di && out.cols == Do, "tdnn_propagate: dims: in.cols=%d Di=%d out.cols=%d Do=%d", in.cols, Di, out.cols, Do);
  TDNNF_REQUIRE(tdnn_rows_ok(&ix, in.rows, out.rows), "tdnn_propagate: input has too few rows for the time offsets");
  TDNNF_REQUIRE(ldw >= ix.num_offsets * Di, "tdnn_propagate: ldw < K*Di");
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

int infer_gemm_f32(void *ctx, hipStream_t s, int role, int comp, const tdnnf_tdnn_indexes &ix, const tdnnf_mat &in, int relu, const float *coef, const tdnnf_mat *add,
                   float add_scale, const int *row_map, const tdnnf_mat &out, bool wants_stats) {
  const tdnnf_net *n = static_cast<const tdnnf_net *>(ctx);
  return gemm_post(ix, in, net_W(n, comp), ix.num_offsets * in.cols, out.cols, in.cols, net_bias(n, comp), relu, coef, add, add_scale, row_map, out, s);
}

int infer_forward(const tdnnf_net *n, const float *coef0, int which, int B, const FwdBuffers &b, tdnnf_mat *out, FwdGemm gemm, void *ctx, hipStream_t s,
                  FwdCounts *counts) {
  const tdnnf_net_config &c = n->cfg;
  const int Hd = c.hidden_dim, L = (int)b.layers.size(), ldH = ldpad(Hd);
  const long long bstride = infer_bn_stride(c);
  auto coef = [&](int i) { return coef0 + i * bstride; };
  const tdnnf_tdnn_indexes ix1 = one_tap();
  FwdCounts cnt = {0, 0, 0, 0};
  auto G = [&](int role, int comp, const tdnnf_tdnn_indexes &ix, const tdnnf_mat &in, int relu, const float *cf, const tdnnf_mat *add, const int *row_map,
               const tdnnf_mat &o, bool wants_stats) {
    cnt.gemms++;
    cnt.rows += o.rows;
    return gemm(ctx, s, role, comp, ix, in, relu, cf, add, add ? c.bypass_scale : 0.f, row_map, o, wants_stats);
  };
  CK(G(0, n->c_lda, ix1, b.lda_in, 0, nullptr, nullptr, nullptr, b.lda_out, true));
  // ---- tdnn1: affine + ReLU + BatchNorm in one GEMM
  CK(G(1, n->tdnn1.comp, ix1, b.lda_out, 1, coef(0), nullptr, nullptr, b.x0, true));
  cnt.fused = 1;
  for (int l = 0; l < L; l++) {
    const FwdLayer &Ly = b.layers[l];
    CK(G(2 + 2 * l, Ly.lin.comp, Ly.lin.ix, Ly.lin_in, 0, nullptr, nullptr, nullptr, Ly.lin_out, true));
    if (Ly.aff.ix.row_stride > 1) {  // (a row order: the sums of squares stay those of the matrix)
      tdnnf_mat po = Ly.perm_out;
      CK(tdnnf_reorder_rows(&Ly.lin_out, B, Ly.aff.ix.row_stride, 1, &po, s));
    }
    if (!Ly.relu.data) {  // noop = Sum(Scale(bypass, input rows), batchnorm(relu(affine))) while the tile is stored
      CK(G(3 + 2 * l, Ly.aff.comp, Ly.aff.ix, Ly.aff_in, 1, coef(1 + l), &Ly.byp, nullptr, Ly.out, true));
      cnt.fused++;
    } else {  // bypass rows strided against the output rows: ReLU in the GEMM, BatchNorm + bypass in the trainer's pass
      CK(G(3 + 2 * l, Ly.aff.comp, Ly.aff.ix, Ly.aff_in, 1, nullptr, nullptr, nullptr, Ly.relu, false));
      const tdnnf_mat x{Ly.relu.data, Ly.out_times, Ly.byp.cols, B * ldH}, ov{Ly.out.data, Ly.out_times, Ly.byp.cols, B * ldH};
      TDNNF_HIP(bn_apply_bypass(view(&x), coef(1 + l), Hd, ldH, view(&Ly.byp), c.bypass_scale, view(&ov), s, nullptr, B));
      cnt.fallback++;
    }
  }
  // ---- the chosen head: prefinal-l, affine + ReLU + batchnorm1, linear + batchnorm2, output
  const auto &H = n->head[which];
  const int r0 = 2 + 2 * L, nb = L + 1;
  CK(G(r0, n->c_prefinal_l, ix1, b.top, 0, nullptr, nullptr, nullptr, b.pl, true));
  CK(G(r0 + 1, H.c_affine, ix1, b.pl, 1, coef(nb), nullptr, nullptr, b.b1, true));
  CK(G(r0 + 2, H.c_linear, ix1, b.b1, 0, coef(nb + 1), nullptr, nullptr, b.b2, true));
  cnt.fused += 2;
  if (which == 0) {  // the rows the map keeps straight into the caller's output
    tdnnf_mat ym = *out;
    ym.rows = b.b2.rows;
    CK(G(r0 + 3, H.c_output, ix1, b.b2, 0, nullptr, nullptr, b.row_map, ym, false));
  } else {
    CK(G(r0 + 3, H.c_output, ix1, b.b2, 0, nullptr, nullptr, nullptr, b.y, false));
    tdnnf_mat lsm = b.lsm;
    CK(tdnnf_log_softmax_propagate(&b.y, &lsm, s));
    TDNNF_HIP(infer_scatter_rows(view(&b.lsm), b.row_map, view(out), s));
  }
  *counts = cnt;
  return TDNNF_OK;
}

}  // namespace tdnnf
