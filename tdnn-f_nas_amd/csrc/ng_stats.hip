// ng_stats.hip -- the statistics side of OnlineNaturalGradient::PreconditionDirections on gfx950 (UPSTREAM Kaldi
// nnet3/natural-gradient-online.{h,cc}; call sites /root/reference/src/nnet3/nnet-tdnn-component.cc:598-599,
// nnet-simple-component.cc:3001-3002; configuration :183-210).  SURVEY.md 8(a) row A8.  ng.h has the file map.
//
// The preconditioned directions are X^ = X - (X W^T) W, returned with scale = sqrt(tr(X X^T) / tr(X^ X^^T)).  What is N-sized
// (N = frames x sequences):
//   every call   H = X W^T                         one pass over X: the MFMA rows GEMM (128x32 tile for R <= 32), the vector-ALU rowdot
//                                                  (ng_valu.hip) or, for taps that are row shifts of one matrix, the one-pass P form
//                tr(X X^T)                         by-product of staging X in that pass
//                L = H^T H,  tr(X^ X^^T) = tr(XX^T) - 2 tr(L) + <L, W W^T>      (R x R, no second pass over X)
//   refresh call J = H^T X, K = J J^T              second pass (first 10 calls, then every update_period-th)
// and then the hand-off to the host (ng_refresh.hip).  X itself is only rewritten by tdnnf_ng_precondition (abi_ng.hip); the trainer
// never materialises X^: it projects the raw gradient (ng_project, ng.h).
#include <string.h>

#include <algorithm>

#include "gemm_f32.h"
#include "ng.h"
#include "ng_kernels.h"

namespace tdnnf {
namespace {

// ------------------------------------------------------------------ workspace layout
// the ||X||^2 partials in front of a statistics workspace, rounded to 64 bytes
size_t part_bytes(int N) { return ((size_t)rows_gemm_sumsq_blocks(N) * sizeof(double) + 63) & ~(size_t)63; }
size_t stats_ws_bytes(int Rp, int Di, int K, int N) {
  return part_bytes(N) + std::max(std::max(wgrad_workspace_bytes(Rp, Rp, 1, N), wgrad_workspace_bytes(Rp, Di, K, N)), ng_pform_ws_bytes(Rp, Di, K, N));
}

// ------------------------------------------------------------------ the P form
constexpr int kPformSpanCap = 4096;  // rows between the first and the last tap (<= 2 x 3 frames x 512 sequences)
struct TapSpan {
  int lo, hi;  // the smallest and the largest row offset of the taps
};
TapSpan tap_span(const tdnnf_tdnn_indexes &ix) {
  TapSpan t{ix.row_offsets[0], ix.row_offsets[0]};
  for (int i = 1; i < ix.num_offsets; i++) {
    t.lo = std::min(t.lo, ix.row_offsets[i]);
    t.hi = std::max(t.hi, ix.row_offsets[i]);
  }
  return t;
}

}  // namespace

// P form of H = X~ W^T for K taps that are row shifts of ONE matrix: P = X [W_0^T | W_1^T | ...] in one pass over X (each row read
// once instead of K times), then H[m] = sum_i P[m + o_i][block i].  Workspace: W's blocks stacked, P, the pass's per-tile ||x||^2.
size_t ng_pform_ws_bytes(int Rp, int Di, int K, int N) {
  if (K < 2 || K * Rp > 64) return 0;
  const size_t M = (size_t)N + kPformSpanCap;
  return sizeof(float) * ((size_t)K * Rp * Di + 64) + sizeof(float) * (M * K * Rp + 64) + sizeof(double) * ((size_t)rows_gemm_sumsq_blocks((int)M) + 8) + 256;
}
// Applies to: taps of one matrix at rows 128 apart in whole tiles (o_i % 128 == 0, N % 128 == 0: the pass's
// per-tile ||x||^2 then add up to each tap's window exactly), no tap coefficients, every row a row of X (row_stride 1), minibatches
// whose passes are bound by the read of X (>= 32 768 rows; below, the K-tap kernel's rows are latency-bound launches either way).
bool ng_pform_ok(int Rp, const NgInput &in, size_t ws_bytes) {
  const int K = in.ix.num_offsets, N = in.N;
  if (!options().ng_pform || K < 2 || K * Rp > 64 || in.eff || in.active || in.ix.row_stride != 1 || N % 128 != 0 || N < 32768) return false;
  const TapSpan sp = tap_span(in.ix);
  for (int i = 0; i < K; i++)
    if ((in.ix.row_offsets[i] - sp.lo) % 128 != 0) return false;
  if (sp.hi - sp.lo > kPformSpanCap || in.Di % 4 != 0 || (in.x.stride % 4) != 0 || in.Di < 1024) return false;  // (narrow matrices -- 160 columns -- measured slower: 78 against 61 us)
  return ws_bytes >= ng_pform_ws_bytes(Rp, in.Di, K, N);
}
int ng_pform_pass(const float *W, int Rp, int ldw, const float *bias, const NgInput &in, float *H, double *part, void *ws, hipStream_t s) {
  const int K = in.ix.num_offsets, N = in.N, Di = in.Di;
  const TapSpan sp = tap_span(in.ix);
  PformTaps tp;
  memset(&tp, 0, sizeof(tp));
  tp.K = K;
  for (int i = 0; i < K; i++) tp.o[i] = in.ix.row_offsets[i] - sp.lo;
  const int M = N + (sp.hi - sp.lo);
  float *WP = (float *)ws;
  float *P = WP + (((size_t)K * Rp * Di + 63) & ~(size_t)63);
  double *psum = (double *)(P + (((size_t)M * K * Rp + 63) & ~(size_t)63));
  hipLaunchKernelGGL(stack_taps_kernel, dim3(grid_for((long long)K * Rp * Di, 256)), dim3(256), 0, s, W, Rp, ldw, Di, K, WP);
  // P = X [W_0^T | W_1^T ...]  (+ ||x||^2 per 128-row tile)
  TDNNF_HIP(rows_gemm_1seg(in.x.data + (size_t)sp.lo * in.x.stride, in.x.stride, WP, Di, true, P, K * Rp, M, K * Rp, Di, 2, nullptr, psum, s));
  hipLaunchKernelGGL(pform_combine_kernel, dim3(N / 128), dim3(256), 0, s, P, K * Rp, tp, Rp, bias, H, N, psum, part,
                     rows_gemm_sumsq_blocks(N));
  TDNNF_HIP(hipGetLastError());
  return TDNNF_OK;
}

// ------------------------------------------------------------------ H = X~ W^T: the two K-tap forms' arguments
RowsGemmArgs ng_pass_gemm_args(const float *W, int ldw, int Rp, const float *bias, const NgInput &in, float *H, int ldh, double *part) {
  const int N = in.N, K = in.ix.num_offsets, Di = in.Di;
  RowsGemmArgs a;
  memset(&a, 0, sizeof(a));
  a.A = in.x.data; a.lda = (long long)in.x.stride * in.ix.row_stride; a.B = W; a.ldb = ldw; a.C = H; a.ldc = ldh; a.M = N; a.N = Rp;
  a.bias = bias;
  a.init_mode = bias ? 1 : 2;
  a.coef = in.eff;
  a.sumsq = part;
  a.nseg = K;
  for (int i = 0; i < K; i++) {
    a.seg[i].a_off = (long long)in.ix.row_offsets[i] * in.x.stride;
    a.seg[i].b_off = (long long)i * Di;
    a.seg[i].klen = Di;
    a.seg[i].m_lo = 0;
    a.seg[i].m_hi = N;
  }
  return a;
}
NgRowdotArgs ng_pass_rowdot_args(const float *WT, int Rp, const float *bias, const NgInput &in, float *H, int ldh, double *part, int part_cap) {
  const int K = in.ix.num_offsets;
  NgRowdotArgs v;
  memset(&v, 0, sizeof(v));
  v.X = in.x.data; v.ldx = in.x.stride; v.row_stride = in.ix.row_stride; v.nseg = K; v.Di = in.Di; v.eff = in.eff; v.WT = WT; v.Rp = Rp;
  v.bias = bias; v.H = H; v.ldh = ldh; v.N = in.N; v.part = part; v.part_cap = part_cap;
  for (int i = 0; i < K; i++) v.seg_off[i] = (long long)in.ix.row_offsets[i] * in.x.stride;
  return v;
}

namespace {

const float *ones_column(const tdnnf_ng *ng, const NgInput &in) { return in.ones ? ng->wlast : nullptr; }

// ------------------------------------------------------------------ first half: everything N x D sized
// What follows H in the first half: the bookkeeping of the call in flight and, on a refresh, J = H^T X.
int stats_after_h(tdnnf_ng *ng, const NgInput &in, const float *H, void *wg_ws, size_t wg_bytes, bool upd, hipStream_t s) {
  const int N = in.N, K = in.ix.num_offsets, Di = in.Di, Rp = ng->Rp, Dp = ng->Dp, D = ng->D;
  ng->cur_upd = upd;
  ng->cur_N = N;
  ng->cur_ones = in.ones;
  if (!upd) return TDNNF_OK;
  TDNNF_REQUIRE(wg_ws && wg_bytes >= wgrad_workspace_bytes(Rp, Di, K, N), "ng: workspace too small");
  TDNNF_HIP(hipMemsetAsync(ng->J, 0, sizeof(float) * (size_t)Rp * Dp, s));
  if (in.ones) TDNNF_HIP(hipMemsetAsync(ng->tmpR, 0, sizeof(float) * Rp, s));
  WgradArgs j;
  memset(&j, 0, sizeof(j));
  j.dY = H; j.lddy = Rp; j.X = in.x.data; j.ldx = in.x.stride; j.Do = Rp; j.Di = Di; j.K = K; j.N = N; j.row_stride = in.ix.row_stride;
  for (int i = 0; i < K; i++) j.row_offsets[i] = in.ix.row_offsets[i];
  j.coef = in.eff; j.scale = 1.f; j.G = ng->J; j.ldg = Dp; j.accumulate = 1; j.bias_acc = in.ones ? ng->tmpR : nullptr;
  j.active = in.active; j.max_active = in.max_active;
  TDNNF_HIP(wgrad(j, wg_ws, wg_bytes, s));  // J = H^T X  (last column: column sums of H)
  if (in.ones) hipLaunchKernelGGL(scatter_col_kernel, dim3((Rp + 63) / 64), dim3(64), 0, s, ng->tmpR, Rp, ng->J, Dp, D - 1);
  return TDNNF_OK;
}

// First half of one PreconditionDirections call: H = X W_t^T (with ||X||^2 per block into `part`) and, on a refresh,
// J = H^T X.  W_t is left untouched.
int stats_main(tdnnf_ng *ng, const NgInput &in, float *H, double *part, void *wg_ws, size_t wg_bytes, bool upd, hipStream_t s) {
  const int N = in.N, K = in.ix.num_offsets, Di = in.Di, Rp = ng->Rp, Dp = ng->Dp;
  const float *bias = ones_column(ng, in);
  // the same product on the vector ALUs, beside the matrix-core GEMMs of the other streams (ng_valu.hip), where its shape allows
  const NgRowdotArgs v = ng_pass_rowdot_args(ng->WT, Rp, bias, in, H, Rp, part, rows_gemm_sumsq_blocks(N));
  const int skip = options().ng_diag_skip;
  if (skip && ng->D != 0 && (((skip & 1) && K == 2 && Di >= 1024) || ((skip & 2) && !(K == 2 && Di >= 1024)))) {
    TDNNF_HIP(hipMemsetAsync(H, 0, sizeof(float) * (size_t)N * Rp, s));
    TDNNF_HIP(hipMemsetAsync(part, 0, sizeof(double) * rows_gemm_sumsq_blocks(N), s));
  } else if (ng_pform_ok(Rp, in, wg_bytes)) {
    int rc = ng_pform_pass(ng->W, Rp, Dp, bias, in, H, part, wg_ws, s);
    if (rc) return rc;
  } else if (options().ng_valu && !in.active && ng_rowdot_ok(v)) {
    TDNNF_HIP(ng_rowdot(v, s));
  } else {
    TDNNF_HIP(rows_gemm(ng_pass_gemm_args(ng->W, Dp, Rp, bias, in, H, Rp, part), true, s));  // H = X W^T (+ ||X||_F^2 per block)
  }
  return stats_after_h(ng, in, H, wg_ws, wg_bytes, upd, s);
}

// ------------------------------------------------------------------ second half: R x R sized and latency bound
// L = H^T H, traces and scale; on a refresh K = J J^T and the hand-off to the host worker.  May run on another stream than
// stats_main as long as it is ordered after it.
int stats_side(tdnnf_ng *ng, const float *H, const double *part, void *wg_ws, size_t wg_bytes, hipStream_t s) {
  const int N = ng->cur_N, Rp = ng->Rp, Dp = ng->Dp;
  TDNNF_REQUIRE(wg_ws && wg_bytes >= wgrad_workspace_bytes(Rp, Rp, 1, N), "ng: workspace too small");
  WgradArgs w;
  memset(&w, 0, sizeof(w));
  w.dY = H; w.lddy = Rp; w.X = H; w.ldx = Rp; w.Do = Rp; w.Di = Rp; w.K = 1; w.N = N; w.row_stride = 1; w.scale = 1.f;
  w.G = ng->Ld; w.ldg = Rp; w.accumulate = 0;
  TDNNF_HIP(wgrad(w, wg_ws, wg_bytes, s));  // L = H^T H
  hipLaunchKernelGGL(ng_scalars_kernel, dim3(1), dim3(256), 0, s, part, rows_gemm_sumsq_blocks(N), ng->cur_ones ? (double)N : 0.0, ng->Ld, ng->WWT,
                     Rp, ng->scal, ng->scale_f);
  if (!ng->cur_upd) return TDNNF_OK;
  TDNNF_HIP(rows_gemm_1seg(ng->J, Dp, ng->J, Dp, true, ng->Kd, Rp, Rp, Rp, Dp, 2, nullptr, nullptr, s));  // K = J J^T
  const size_t fRR = (size_t)Rp * Rp;
  TDNNF_HIP(hipMemcpyAsync(ng->h_K, ng->Kd, sizeof(float) * fRR, hipMemcpyDeviceToHost, s));
  TDNNF_HIP(hipMemcpyAsync(ng->h_L, ng->Ld, sizeof(float) * fRR, hipMemcpyDeviceToHost, s));
  TDNNF_HIP(hipMemcpyAsync(ng->h_tr0, ng->scal, sizeof(double), hipMemcpyDeviceToHost, s));
  TDNNF_HIP(hipEventRecord(ng->ev_job, s));
  ng_refresh_submit(ng, N, ng->ev_job);
  return TDNNF_OK;
}

// both halves on one stream; ws = [sumsq partials | wgrad workspace]
int stats_core(tdnnf_ng *ng, const NgInput &in, float *H, void *ws, size_t ws_bytes, bool upd, hipStream_t s) {
  TDNNF_REQUIRE(ws && ws_bytes >= stats_ws_bytes(ng->Rp, in.Di, in.ix.num_offsets, in.N), "ng: workspace too small");
  double *part = (double *)ws;
  void *wg_ws = (char *)ws + part_bytes(in.N);
  const size_t wg_bytes = ws_bytes - part_bytes(in.N);
  int rc = stats_main(ng, in, H, part, wg_ws, wg_bytes, upd, s);
  if (rc) return rc;
  return stats_side(ng, H, part, wg_ws, wg_bytes, s);
}

// Init(): default state, then self-training on this minibatch (3 refreshes from the same data), all on stream s
int init_from(tdnnf_ng *ng, const NgInput &in, int D, float *H, void *ws, size_t ws_bytes, hipStream_t s) {
  int rc = ng_init_default(ng, D, s);
  if (rc) return rc;
  if (ng->rank > 0) {
    const int iters = in.N <= ng->rank ? 1 : 3;
    for (int i = 0; i < iters; i++) {
      if ((rc = stats_core(ng, in, H, ws, ws_bytes, true, s))) return rc;
      if ((rc = ng_finalize(ng, s))) return rc;
    }
  }
  ng->t = 0;
  return TDNNF_OK;
}

// ------------------------------------------------------------------ what the entries that start a call on an object share
int input_dim(const NgInput &in) { return in.ix.num_offsets * in.Di + (in.ones ? 1 : 0); }

// An entry whose caller brings the data and a full statistics workspace lets an object be initialised from its first minibatch.
struct NgFirstUse {
  const NgInput &in;
  float *H;
  void *ws;
  size_t ws_bytes;
};
// First use (where the entry allows it), the dimension check, no call in flight (where the entry says so), and the second half of a
// refresh the previous call on this object started.  A rank-0 object has nothing pending: its entries return behind this.
int begin_call(tdnnf_ng *ng, int D, const NgFirstUse *first, bool reset_cur_N, hipStream_t s) {
  if (ng->D == 0 && first) {
    int rc = init_from(ng, first->in, D, first->H, first->ws, first->ws_bytes, s);
    if (rc) return rc;
  }
  TDNNF_REQUIRE(ng->D == D, "ng: dimension changed from %d to %d", ng->D, D);
  if (reset_cur_N) ng->cur_N = 0;
  return ng_finalize(ng, s);
}

}  // namespace

size_t ng_stats_workspace_bytes(int rank, int D, int K, int N) {
  const int Rp = pad4(std::max(1, std::min(rank, D - 1)));
  const int Di = K > 0 ? D / K : D;
  return stats_ws_bytes(Rp, Di, std::max(K, 1), N) + 64;
}
int ng_dim(const tdnnf_ng *ng) { return ng->D; }

// (the one entry that leaves cur_N alone: both halves run inside it)
int ng_stats_step(tdnnf_ng *ng, const NgInput &in, float *H, void *ws, size_t ws_bytes, hipStream_t s) {
  const int K = in.ix.num_offsets;
  TDNNF_REQUIRE(ng && H && in.N > 0 && K >= 1 && K <= kMaxSeg && in.Di > 0, "ng_stats_step: bad arguments");
  NgCallScope scope;
  const NgFirstUse first{in, H, ws, ws_bytes};
  int rc = begin_call(ng, input_dim(in), &first, false, s);
  if (rc || ng->rank == 0) return rc;
  rc = stats_core(ng, in, H, ws, ws_bytes, ng_updating(ng), s);
  ng->t += 1;
  return rc;
}

int ng_stats_main(tdnnf_ng *ng, const NgInput &in, float *H, double *part, void *ws, size_t ws_bytes, hipStream_t s) {
  const int K = in.ix.num_offsets;
  TDNNF_REQUIRE(ng && H && part && in.N > 0 && K >= 1 && K <= kMaxSeg && in.Di > 0, "ng_stats_main: bad arguments");
  NgCallScope scope;
  const NgFirstUse first{in, H, ws, ws_bytes};
  int rc = begin_call(ng, input_dim(in), &first, true, s);
  if (rc || ng->rank == 0) return rc;
  return stats_main(ng, in, H, part, ws, ws_bytes, ng_updating(ng), s);
}

// (no first use: the object must be initialised, which its argument check says in its own words; rank 0 returns ahead of the scope)
int ng_stats_main_prepare(tdnnf_ng *ng, const NgInput &in, float *H, double *part, hipStream_t s, RowsGemmArgs *out) {
  const int K = in.ix.num_offsets, D = input_dim(in);
  TDNNF_REQUIRE(ng && H && part && out && in.N > 0 && K >= 1 && K <= kMaxSeg && ng->D == D, "ng_stats_main_prepare: bad arguments");
  if (ng->rank == 0) {  // nothing to precondition: no pass (out->M = 0 fails rows_gemm_group_ok, the caller leaves the object to its own call)
    memset(out, 0, sizeof(*out));
    ng->cur_N = 0;
    return TDNNF_OK;
  }
  NgCallScope scope;
  int rc = begin_call(ng, D, nullptr, true, s);
  if (rc) return rc;
  *out = ng_pass_gemm_args(ng->W, ng->Dp, ng->Rp, ones_column(ng, in), in, H, ng->Rp, part);
  return TDNNF_OK;
}
// (also the second half of ng_external_begin)
int ng_stats_main_finish(tdnnf_ng *ng, const NgInput &in, const float *H, void *ws, size_t ws_bytes, hipStream_t s) {
  TDNNF_REQUIRE(ng && H && ng->D != 0 && ng->rank > 0 && in.N > 0, "ng_stats_main_finish: bad arguments");
  NgCallScope scope;
  return stats_after_h(ng, in, H, ws, ws_bytes, ng_updating(ng), s);
}

// (no first use: before it, and for rank 0, *W stays null and nothing else happens -- no dimension check, cur_N as it was.  No
// NgCallScope either: a refresh completed here runs its two GEMMs in the caller's arithmetic and profiler class)
int ng_external_begin(tdnnf_ng *ng, int D, const float **W, int *Rp, int *ldw, hipStream_t s) {
  TDNNF_REQUIRE(ng && W && Rp && ldw, "ng_external_begin: bad arguments");
  *W = nullptr;
  if (ng->D == 0 || ng->rank == 0) return TDNNF_OK;  // first minibatch (W_0 comes from the data) / nothing to precondition
  int rc = begin_call(ng, D, nullptr, true, s);
  if (rc) return rc;
  *W = ng->W;
  *Rp = ng->Rp;
  *ldw = ng->Dp;
  return TDNNF_OK;
}

int ng_stats_side(tdnnf_ng *ng, const float *H, const double *part, void *ws, size_t ws_bytes, hipStream_t s) {
  TDNNF_REQUIRE(ng && H && part, "ng_stats_side: bad arguments");
  if (ng->rank == 0 || ng->cur_N == 0) return TDNNF_OK;
  NgCallScope scope;
  int rc = stats_side(ng, H, part, ws, ws_bytes, s);
  ng->t += 1;
  return rc;
}

// ------------------------------------------------------------------ the rank-R projections of the raw gradient
size_t ng_project_tmp_floats(const tdnnf_ng *in, const tdnnf_ng *out, int Do, int ldT) {
  const size_t q = in ? (size_t)Do * in->Rp : 0, p = out ? (size_t)out->Rp * ldT : 0;
  return std::max(q, p) + 16;
}

int ng_project(tdnnf_ng *in, tdnnf_ng *out, float *T, int Do, int Dx, int ldT, float *tmp, hipStream_t s) {
  TDNNF_REQUIRE(T && tmp && ldT % 4 == 0 && ldT >= Dx, "ng_project: bad arguments");
  NgCallScope scope;
  if (in && in->rank > 0) {
    TDNNF_REQUIRE(in->D == Dx && in->Dp == ldT, "ng_project: input-side dimension mismatch");
    const int Rp = in->Rp;
    TDNNF_HIP(rows_gemm_1seg(T, ldT, in->W, in->Dp, true, tmp, Rp, Do, Rp, ldT, 2, nullptr, nullptr, s));        // Q = T Wx^T
    TDNNF_HIP(rows_gemm_1seg(tmp, Rp, in->W, in->Dp, false, T, ldT, Do, ldT, Rp, 0, in->neg_one, nullptr, s));    // T -= Q Wx
  }
  if (out && out->rank > 0) {
    TDNNF_REQUIRE(out->D == Do, "ng_project: output-side dimension mismatch");
    const int Rp = out->Rp;
    TDNNF_HIP(rows_gemm_1seg(out->W, out->Dp, T, ldT, false, tmp, ldT, Rp, ldT, Do, 2, nullptr, nullptr, s));     // P = Wy T
    TDNNF_HIP(rows_gemm_1seg(out->WT, Rp, tmp, ldT, false, T, ldT, Do, ldT, Rp, 0, out->neg_one, nullptr, s));    // T -= Wy^T P
  }
  return TDNNF_OK;
}

// ------------------------------------------------------------------ the per-object chain (ng.h)
void ng_set_column(const float *v, int rows, float *T, int ldT, int col, hipStream_t s) {
  hipLaunchKernelGGL(set_column_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, v, rows, T, ldT, col);
}

int ng_chain_one(tdnnf_ng *in, tdnnf_ng *out, const float *H_in, const double *part_in, const float *H_out, const double *part_out, float *T, int Do,
                 int Dx, int ldT, int ldw, float *W_acc, float *bias_acc, void *side_ws, size_t side_ws_bytes, float *tmp, hipStream_t s) {
  int rc = ng_stats_side(in, H_in, part_in, side_ws, side_ws_bytes, s);
  if (rc) return rc;
  if ((rc = ng_stats_side(out, H_out, part_out, side_ws, side_ws_bytes, s))) return rc;
  if ((rc = ng_project(in, out, T, Do, Dx, ldT, tmp, s))) return rc;
  hipLaunchKernelGGL(ng_commit_kernel, dim3(grid_for((long long)Do * Dx, 256)), dim3(256), 0, s, T, ldT, Do, ldw, in->scale_f, out->scale_f, W_acc,
                     bias_acc);
  return TDNNF_OK;
}

}  // namespace tdnnf
