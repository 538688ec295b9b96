// abi_ng.hip -- the OnlineNaturalGradient object behind the C-ABI (include/tdnnf_hip.h): create / freeze / destroy, the
// component-level entry point tdnnf_ng_precondition (UPSTREAM Kaldi nnet3/natural-gradient-online.{h,cc}, PreconditionDirections:
// X is replaced by X^) and the stand-alone statistics pass tdnnf_ng_stats_pass.  The algorithm is in ng_stats.hip and ng_refresh.hip.
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "gemm_f32.h"
#include "ng.h"

using namespace tdnnf;

extern "C" {

const float *tdnnf_ng_scale_dev(const tdnnf_ng *ng) { return ng && ng->dev ? ng->scale_f : nullptr; }

size_t tdnnf_ng_stats_pass_workspace_bytes(int rank, int Di, int num_taps, int N) { return ng_pform_ws_bytes(pad4(rank), Di, num_taps, N) + 64; }

int tdnnf_ng_stats_pass(const tdnnf_tdnn_indexes *ix, const tdnnf_mat *X, int Di, const float *eff, const float *WT, const float *W, int ldw,
                        const float *bias, tdnnf_mat *H, double *sumsq, int sumsq_cap, int use_valu, void *workspace, size_t workspace_bytes,
                        tdnnf_stream stream) {
  TDNNF_REQUIRE(ix && X && X->data && H && H->data && Di > 0 && ix->num_offsets >= 1 && ix->num_offsets <= kMaxSeg && ix->row_stride >= 1,
                "ng_stats_pass: bad arguments");
  const int K = ix->num_offsets, N = H->rows, Rp = H->cols;
  for (int i = 0; i < K; i++)
    TDNNF_REQUIRE(ix->row_offsets[i] >= 0 && (long long)(N - 1) * ix->row_stride + ix->row_offsets[i] < X->rows && Di <= X->cols,
                  "ng_stats_pass: tap %d reads outside X (%d x %d)", i, X->rows, X->cols);
  TDNNF_REQUIRE(!sumsq || sumsq_cap >= rows_gemm_sumsq_blocks(N), "ng_stats_pass: sumsq needs %d entries", rows_gemm_sumsq_blocks(N));
  hipStream_t s = (hipStream_t)stream;
  NgInput in;
  memset(&in, 0, sizeof(in));
  in.x = view(X); in.ix = *ix; in.Di = Di; in.ones = bias ? 1 : 0; in.N = N; in.eff = eff;
  if (use_valu == 2) {  // the P form: one pass over X for all taps
    TDNNF_REQUIRE(W && ldw >= K * Di && sumsq && H->stride == Rp && workspace && ng_pform_ok(Rp, in, workspace_bytes),
                  "ng_stats_pass: the one-pass form takes >= 2 taps of one matrix whole 128-row tiles apart, N %% 128 == 0, N >= 32768, taps x rank <= 64, no coefficients");
    return ng_pform_pass(W, Rp, ldw, bias, in, H->data, sumsq, workspace, s);
  }
  if (use_valu) {
    const NgRowdotArgs v = ng_pass_rowdot_args(WT, Rp, bias, in, H->data, H->stride, sumsq, sumsq_cap);
    TDNNF_REQUIRE(WT && ng_rowdot_ok(v), "ng_stats_pass: the vector-ALU kernel takes rank 20 / 40 / 80 and 16-byte aligned rows");
    TDNNF_HIP(ng_rowdot(v, s));
    return TDNNF_OK;
  }
  TDNNF_REQUIRE(W && ldw >= K * Di, "ng_stats_pass: the MFMA form needs W (rank x ldw)");
  GemmPrecisionScope exact_f32(2);
  TDNNF_HIP(rows_gemm(ng_pass_gemm_args(W, ldw, Rp, bias, in, H->data, H->stride, sumsq), true, s));
  return TDNNF_OK;
}

int tdnnf_ng_create(int rank, int update_period, float num_samples_history, float alpha, tdnnf_ng **out) {
  TDNNF_REQUIRE(out && rank >= 0 && update_period >= 1 && num_samples_history > 0 && alpha >= 0, "ng_create: bad configuration");
  tdnnf_ng *ng = new tdnnf_ng();
  ng->rank = rank;
  ng->Rp = 0;
  ng->update_period = update_period;
  ng->t = 0;
  ng->D = ng->Dp = 0;
  ng->frozen = 0;
  ng->num_samples_history = num_samples_history;
  ng->alpha = alpha;
  ng->epsilon = 1.0e-10f;
  ng->delta = 5.0e-04f;
  ng->rho = 0;
  ng->dev = nullptr;
  ng->pin = nullptr;
  ng->scratch = nullptr;
  ng->scratch_floats = 0;
  ng->pending = 0;
  ng->job_done = 0;
  ng->ev_job = nullptr;
  ng->ev_wait = nullptr;
  ng->must_reorth = false;
  *out = ng;
  return TDNNF_OK;
}

// OnlineNaturalGradient::Freeze (UPSTREAM; called by FreezeNaturalGradient, /root/reference/src/nnet3/nnet-tdnn-component.cc:979-982):
// a frozen object keeps preconditioning with its current state and never refreshes it
int tdnnf_ng_freeze(tdnnf_ng *ng, int freeze) {
  TDNNF_REQUIRE(ng, "ng_freeze: null object");
  ng->frozen = freeze ? 1 : 0;
  return TDNNF_OK;
}

void tdnnf_ng_destroy(tdnnf_ng *ng) {
  if (!ng) return;
  if (ng->pending) ng_pool_wait(ng);  // the worker still reads this object's pinned buffers
  hipFree(ng->dev);
  hipHostFree(ng->pin);
  hipFree(ng->scratch);
  if (ng->ev_job) hipEventDestroy(ng->ev_job);
  delete ng;
}

// Component-level entry point: X (N x D, device) is replaced by X^; *scale_host (optional) receives the scale,
// which costs a stream synchronisation.
int tdnnf_ng_precondition(tdnnf_ng *ng, tdnnf_mat *X, float *scale_host, tdnnf_stream stream) {
  TDNNF_REQUIRE(ng && mat_ok(X) && X->rows > 0 && X->cols > 0, "ng_precondition: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  NgCallScope scope;
  if (X->cols == 1) {  // preconditioning one column is pointless (UPSTREAM)
    if (scale_host) *scale_host = 1.0f;
    return TDNNF_OK;
  }
  const int N = X->rows, D = X->cols;
  const int Rp = pad4(std::max(1, std::min(ng->rank, D - 1)));
  const size_t ws_bytes = ng_stats_workspace_bytes(ng->rank, D, 1, N);
  const size_t need = (size_t)N * Rp + ws_bytes / sizeof(float) + 64;
  if (ng->scratch_floats < need) {
    if (ng->scratch) hipFree(ng->scratch);
    ng->scratch = nullptr;
    ng->scratch_floats = 0;
    TDNNF_HIP(hipMalloc((void **)&ng->scratch, sizeof(float) * need));
    ng->scratch_floats = need;
  }
  float *H = ng->scratch;
  void *ws = (void *)(((uintptr_t)(H + (size_t)N * Rp) + 63) & ~(uintptr_t)63);
  NgInput in;
  memset(&in, 0, sizeof(in));
  in.x = view(X);
  in.ix.row_stride = 1;
  in.ix.num_offsets = 1;
  in.Di = D;
  in.N = N;
  int rc = ng_stats_step(ng, in, H, ws, ws_bytes - 64, s);
  if (rc) return rc;
  if (ng->rank == 0) {
    if (scale_host) *scale_host = 1.0f;
    return TDNNF_OK;
  }
  TDNNF_HIP(rows_gemm_1seg(H, ng->Rp, ng->W, ng->Dp, false, X->data, X->stride, N, D, ng->Rp, 0, ng->neg_one, nullptr, s));  // X^ = X - H W
  if (scale_host) {
    TDNNF_HIP(hipMemcpyAsync(ng->h_scale, ng->scale_f, sizeof(float), hipMemcpyDeviceToHost, s));
    TDNNF_HIP(hipStreamSynchronize(s));
    *scale_host = *ng->h_scale;
  }
  return TDNNF_OK;
}

}  // extern "C"
