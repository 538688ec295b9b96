// chain_num.hip -- the numerator of the chain objective (log domain; one wave per sequence for narrow supervisions, num_wide_kernels.h for
// wide ones), the kernels that finish the objective (sum, l2 term, failure path) and the entry point that runs all three parts.
// Denominator: chain_den.hip.  An end-to-end supervision (kind 1: one cyclic graph per sequence) takes the kernels of chain_num_e2e.hip
// instead: the host functions here dispatch on the kind, everything else -- zero-fill, l2 term, finish, failure path -- is shared.
#include <math.h>

#include <algorithm>

#include "chain_plan.h"

namespace tdnnf {
namespace {

// The numerator recursion runs in the log domain, where the values grow with the frame index (log alpha ~ -8 t): at 500
// frames a float's 24 bits leave an absolute error of ~2e-4 in the exponent of a posterior, 2e-3 in the posteriors of a
// 1500-frame chunk (measured: frame sums of gamma_num off by up to 2.2e-3, derivative 6.8e-4 from a float64 evaluation).  Doubles:
// one wave per sequence walks a few states per frame, the arithmetic is free.
__device__ __forceinline__ double log_add(double a, double b) {
  if (a == -INFINITY) return b;
  if (b == -INFINITY) return a;
  const double m = fmax(a, b), d = fmin(a, b) - m;
  return m + log1p(exp(d));
}

// one wave per sequence.  la/lb: global scratch indexed by global state id.
__global__ __launch_bounds__(64) void numerator_kernel(SupDev sp, MatView y, MatView xent_out, double *la, double *lb,
                                                       double *num_logprob, double *xent_objf, MatView deriv,
                                                       MatView xent_deriv, float xent_scale, int phases) {
  // phases bit 0: forward-backward recursion (la, lb, total -> num_logprob): needs the chain output y only;
  //        bit 2: xent posteriors / objective; bit 1: deriv += weight * gamma_num  (both need the recursion's la / lb / total,
  //        possibly from an earlier launch)
  const int s = blockIdx.x, lane = threadIdx.x, B = sp.B, T = sp.T;
  const int *fsb = sp.frame_state_begin + (size_t)s * (T + 2);
  const int s0 = sp.seq_state_begin[s], s1 = sp.seq_state_begin[s + 1];
  double tot = -INFINITY;
  if (phases & 1) {
  for (int i = s0 + lane; i < s1; i += 64) la[i] = (i == s0) ? 0.0 : -INFINITY;
  __syncthreads();
  for (int t = 1; t <= T; t++) {  // states entered at time t
    for (int st = fsb[t] + lane; st < fsb[t + 1]; st += 64) {
      double v = -INFINITY;
      for (int a = sp.in_begin[st]; a < sp.in_begin[st + 1]; a++)
        v = log_add(v, la[sp.in_src[a]] + ((double)sp.in_lp[a] + (double)y.data[(size_t)((t - 1) * B + s) * y.stride + sp.in_pdf[a]]));
      la[st] = v;
    }
    __syncthreads();
  }
  for (int st = fsb[T] + lane; st < fsb[T + 1]; st += 64) {
    const float f = sp.final_logprob[st];
    lb[st] = (double)f;
    if (f != -INFINITY) tot = log_add(tot, la[st] + (double)f);
  }
  for (int o = 32; o > 0; o >>= 1) tot = log_add(tot, __shfl_xor(tot, o, 64));
  __syncthreads();
  for (int t = T - 1; t >= 0; t--) {
    for (int st = fsb[t] + lane; st < fsb[t + 1]; st += 64) {
      double v = -INFINITY;
      for (int a = sp.out_begin[st]; a < sp.out_begin[st + 1]; a++)
        v = log_add(v, ((double)sp.out_lp[a] + (double)y.data[(size_t)(t * B + s) * y.stride + sp.out_pdf[a]]) + lb[sp.out_dst[a]]);
      lb[st] = v;
    }
    __syncthreads();
  }
  } else {
    tot = num_logprob[s];
  }
  const bool do_xent = (phases & 4) != 0, do_deriv = (phases & 2) != 0;
  if ((phases & 1) && lane == 0) num_logprob[s] = tot;
  // posteriors: lane = frame (distinct output rows per lane, fixed arc order -> deterministic)
  double xo = 0.0;
  for (int t = lane; t < T; t += 64) {
    const size_t row = (size_t)(t * B + s);
    for (int st = fsb[t]; st < fsb[t + 1]; st++)
      for (int a = sp.out_begin[st]; a < sp.out_begin[st + 1]; a++) {
        const int pdf = sp.out_pdf[a];
        const double ll = (double)sp.out_lp[a] + (double)y.data[row * y.stride + pdf];
        const float gam = sp.weight * (float)exp(la[st] + ll + lb[sp.out_dst[a]] - tot);
        if (do_deriv && deriv.data) deriv.data[row * deriv.stride + pdf] += gam;
        if (do_xent && xent_deriv.data) xent_deriv.data[row * xent_deriv.stride + pdf] += xent_scale * gam;
        if (do_xent && xent_out.data) xo += (double)gam * (double)xent_out.data[row * xent_out.stride + pdf];
      }
  }
  if (do_xent) {
    for (int o = 32; o > 0; o >>= 1) xo += __shfl_xor(xo, o, 64);
    if (lane == 0) xent_objf[s] = xo;
  }
}

// results: [0] objf [1] l2_term [2] weight [3] num [4] den [5] ok [6] xent objf
__global__ void chain_finalize_kernel(const double *num_lp, const double *den_lp, const double *xent, const double *l2sum,
                                      int B, int T, float weight, float l2_regularize, double *results) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double num = 0, den = 0, xo = 0;
  for (int s = 0; s < B; s++) {
    num += num_lp[s];
    den += den_lp[s];
    xo += xent[s];
  }
  num *= weight;
  den *= weight;
  double objf = num - den;
  const double w = (double)weight * B * T;
  const bool ok = (objf - objf == 0.0);
  if (!ok) objf = -10.0 * w;
  results[0] = objf;
  results[1] = (l2_regularize == 0.f || !l2sum) ? 0.0 : -0.5 * (double)weight * l2_regularize * l2sum[0];
  results[2] = w;
  results[3] = num;
  results[4] = den;
  results[5] = ok ? 1.0 : 0.0;
  results[6] = ok ? xo : 0.0;
}

// failure path (objf not finite): zero the derivatives; otherwise add the l2 term's derivative.
__global__ void chain_guard_kernel(const double *results, MatView y, float l2_scale, MatView d, MatView xd) {
  const bool ok = results[5] != 0.0;
  if (ok && l2_scale == 0.f) return;
  const long long total = (long long)d.rows * d.cols;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int r = (int)(e / d.cols), c = (int)(e % d.cols);
    if (!ok) {
      d.data[(size_t)r * d.stride + c] = 0.f;
      if (xd.data) xd.data[(size_t)r * xd.stride + c] = 0.f;
    } else {
      d.data[(size_t)r * d.stride + c] += -l2_scale * y.data[(size_t)r * y.stride + c];
    }
  }
}
// the l2 term's sum of squares without atomics (the term has the same bits on every call): part[block], then their sum in order.  Until the
// end-to-end supervision came, chain_finish added per-block sums with atomicAdd on a double, in the order the blocks arrived: the term's
// last bits differed between two calls on the same inputs (1 - 4 ulps, tests/test_gpu_chain_e2e.py), which no two calls can then be
// compared by.  tdnnf_chain_objf always summed this way.
__global__ __launch_bounds__(1024) void sumsq_parts_kernel(MatView y, double *part) {
  __shared__ double red[16];
  double s = 0;
  const long long total = (long long)y.rows * y.cols;
  for (long long e = blockIdx.x * 1024LL + threadIdx.x; e < total; e += gridDim.x * 1024LL) {
    const double v = y.data[(size_t)(e / y.cols) * y.stride + e % y.cols];
    s += v * v;
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0;
    for (int w = 0; w < 16; w++) t += red[w];
    part[blockIdx.x] = t;
  }
}
__global__ void sum_parts_kernel(const double *part, int n, double *out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double t = 0;
  for (int i = 0; i < n; i++) t += part[i];
  out[0] = t;
}
__global__ void zero_rows_kernel(MatView m) {
  const long long total = (long long)m.rows * m.cols;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL)
    m.data[(size_t)(e / m.cols) * m.stride + e % m.cols] = 0.f;
}

}  // namespace
}  // namespace tdnnf

#include "num_wide_kernels.h"

namespace tdnnf {
namespace {

// Which form a call takes and on which scratch.  A wide supervision (chain_types.h) owns its log alpha / log beta, a narrow one uses the
// workspace's; both forms write the same values there, so the three parts of one minibatch need not take the same form.
struct NumCall {
  bool wide_form;
  double *la, *lb;
};
int num_call(const tdnnf_supervision *sp, const ChainBufs &b, NumCall *c) {
  const int form = options().num_form;
  c->wide_form = form == 2 || (form != 1 && sp->wide);
  TDNNF_REQUIRE(!c->wide_form || sp->pf_src, "chain numerator: option num_form = 2 needs a supervision that was created under it (or a wide one)");
  c->la = sp->wide ? sp->la_own : b.la;
  c->lb = sp->wide ? sp->lb_own : b.lb;
  return TDNNF_OK;
}

template <int NT>
int num_wide_recursion(const tdnnf_supervision *sp, const MatView &y, const NumCall &c, double *num_lp, hipStream_t s) {
  const int W = std::max(sp->max_states_per_frame, 1), A = std::max(sp->max_arcs_per_frame, 1), cap = options().num_frontier_cap;
  const size_t lds = num_wide_lds(W, A, sp->T);
  if (lds > kLdsBudget || (cap > 0 && W > cap)) {  // the frontier in global memory: no width is refused
    hipLaunchKernelGGL(num_wide_recursion_global_kernel<NT>, dim3(sp->B), dim3(NT), 0, s, sup_dev(sp), y, c.la, c.lb, num_lp);
    return TDNNF_OK;
  }
  TDNNF_HIP(hipFuncSetAttribute((const void *)num_wide_recursion_kernel<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(num_wide_recursion_kernel<NT>, dim3(sp->B), dim3(NT), lds, s, sup_dev(sp), y, c.la, c.lb, num_lp, W, A);
  return TDNNF_OK;
}

// posteriors of the wide form: deriv and / or xent_deriv, the xent objective when do_xent
void num_wide_posteriors(const tdnnf_supervision *sp, const MatView &y, const MatView &xent_out, const NumCall &c, const ChainBufs &b, const MatView &deriv,
                         const MatView &xent_deriv, float xent_scale, bool do_xent, hipStream_t s) {
  const int blocks = (sp->T + kNumWideFrames - 1) / kNumWideFrames;
  hipLaunchKernelGGL(num_wide_posterior_kernel, dim3(blocks, sp->B), dim3(kNumWidePostThreads), 0, s, sup_dev(sp), sup_wide_dev(sp), y, xent_out, c.la, c.lb,
                     b.num_lp, deriv, xent_deriv, xent_scale, do_xent ? 1 : 0);
  if (do_xent) hipLaunchKernelGGL(num_wide_xent_sum_kernel, dim3((sp->B + 63) / 64), dim3(64), 0, s, sp->xent_part, sp->B, blocks, b.xent);
}

}  // namespace

float chain_supervision_weight(const tdnnf_supervision *sp) { return sp->weight; }
bool chain_supervision_needs_assign(const tdnnf_supervision *sp) { return sp->ts_reserved && sp->ts_assigns == 0; }
int sup_need_minibatch(const tdnnf_supervision *sp, const char *who) {
  TDNNF_REQUIRE(!sp->e2e_reserved || sp->e2e_assigns > 0, "%sthe reserved supervision holds no minibatch yet (tdnnf_supervision_assign_e2e gives it one)", who);
  TDNNF_REQUIRE(!sp->ts_reserved || sp->ts_assigns > 0, "%sthe reserved supervision holds no minibatch yet (tdnnf_supervision_assign gives it one)", who);
  return TDNNF_OK;
}
// (2) numerator recursion; xent_deriv = xent_regularize * gamma_num, xent objective -> workspace.  Does not touch deriv.
// In two launchable halves: the recursion needs the chain output only (the trainer starts it beside the denominator, under the
// xent head's forward pass: 1.35 ms of one wave per sequence walking 2 x 500 dependent frames that the step otherwise waited for),
// the xent posteriors need the recursion and the xent head's log-softmax.
namespace {
// forward_only (tdnnf_chain_objf without an xent_output): an end-to-end supervision keeps nothing per frame; the other kind runs as ever
int num_recursion(const tdnnf_supervision *sp, const tdnnf_mat *y, const ChainBufs &b, hipStream_t s, bool forward_only = false) {
  if (sp->kind == 1) return num_e2e_recursion(sp, view(y), b.num_lp, forward_only, s);
  const int B = sp->B;
  const MatView none{nullptr, 0, 0, 0};
  NumCall c;
  int rc = num_call(sp, b, &c);
  if (rc) return rc;
  if (c.wide_form) {
    if ((rc = sp->max_states_per_frame <= 64 ? num_wide_recursion<64>(sp, view(y), c, b.num_lp, s) : num_wide_recursion<256>(sp, view(y), c, b.num_lp, s))) return rc;
  } else {
    hipLaunchKernelGGL(numerator_kernel, dim3(B), dim3(64), 0, s, sup_dev(sp), view(y), none, c.la, c.lb, b.num_lp, b.xent, none, none, 0.f, 1);
  }
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}
int num_xent(const tdnnf_supervision *sp, const tdnnf_mat *y, const tdnnf_mat *xent_output, float xent_regularize, tdnnf_mat *xent_deriv, const ChainBufs &b,
             hipStream_t s, bool xent_deriv_initialised) {
  const int B = sp->B;
  MatView yv = view(y);
  MatView xdv = xent_deriv ? view(xent_deriv) : MatView{nullptr, 0, 0, 0};
  MatView xov = xent_output ? view(xent_output) : MatView{nullptr, 0, 0, 0};
  if (xent_deriv && !xent_deriv_initialised) {  // (initialised: the posteriors are added onto what the caller put there)
    if (xdv.stride == xdv.cols) TDNNF_HIP(hipMemsetAsync(xdv.data, 0, sizeof(float) * (size_t)xdv.rows * xdv.cols, s));  // one contiguous fill
    else hipLaunchKernelGGL(zero_rows_kernel, dim3(grid_for((long long)xdv.rows * xdv.cols, 256)), dim3(256), 0, s, xdv);
  }
  if (sp->kind == 1) return num_e2e_posteriors(sp, yv, xov, b.num_lp, b.xent, MatView{nullptr, 0, 0, 0}, xdv, xent_regularize, true, s);
  NumCall c;
  int rc = num_call(sp, b, &c);
  if (rc) return rc;
  if (c.wide_form) num_wide_posteriors(sp, yv, xov, c, b, MatView{nullptr, 0, 0, 0}, xdv, xent_regularize, true, s);
  else
    hipLaunchKernelGGL(numerator_kernel, dim3(B), dim3(64), 0, s, sup_dev(sp), yv, xov, c.la, c.lb, b.num_lp, b.xent, MatView{nullptr, 0, 0, 0},
                       xdv, xent_regularize, 4);
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}
}  // namespace
int chain_num_recursion(const tdnnf_supervision *sp, const tdnnf_den_graph *g, const tdnnf_mat *y, void *ws, hipStream_t s) {
  return num_recursion(sp, y, chain_bufs(g, sp->B, sp->T, ws), s);
}
int chain_num_xent(const tdnnf_den_graph *g, const tdnnf_supervision *sp, const tdnnf_mat *y, const tdnnf_mat *xent_output, float xent_regularize,
                   tdnnf_mat *xent_deriv, void *ws, hipStream_t s, bool xent_deriv_initialised) {
  return num_xent(sp, y, xent_output, xent_regularize, xent_deriv, chain_bufs(g, sp->B, sp->T, ws), s, xent_deriv_initialised);
}
int chain_num(const tdnnf_den_graph *g, const tdnnf_supervision *sp, const tdnnf_mat *y, const tdnnf_mat *xent_output,
              float xent_regularize, tdnnf_mat *xent_deriv, void *ws, hipStream_t s, bool xent_deriv_initialised) {
  int rc = chain_num_recursion(sp, g, y, ws, s);
  if (rc) return rc;
  return chain_num_xent(g, sp, y, xent_output, xent_regularize, xent_deriv, ws, s, xent_deriv_initialised);
}
// (3) after (1) and (2): deriv += weight * gamma_num; objective, l2 term, failure handling
int chain_finish(const tdnnf_den_graph *g, const tdnnf_supervision *sp, const tdnnf_mat *y, float l2_regularize, double *results,
                 tdnnf_mat *deriv, tdnnf_mat *xent_deriv, void *ws, hipStream_t s) {
  const int B = sp->B, T = sp->T;
  ChainBufs b = chain_bufs(g, B, T, ws);
  MatView yv = view(y), dv = view(deriv);
  MatView xdv = xent_deriv ? view(xent_deriv) : MatView{nullptr, 0, 0, 0};
  const MatView none{nullptr, 0, 0, 0};
  int rc;
  if (sp->kind == 1) {
    if ((rc = num_e2e_posteriors(sp, yv, none, b.num_lp, b.xent, dv, none, 0.f, false, s))) return rc;
  } else {
    NumCall c;
    if ((rc = num_call(sp, b, &c))) return rc;
    if (c.wide_form) num_wide_posteriors(sp, yv, none, c, b, dv, none, 0.f, false, s);
    else hipLaunchKernelGGL(numerator_kernel, dim3(B), dim3(64), 0, s, sup_dev(sp), yv, none, c.la, c.lb, b.num_lp, b.xent, dv, none, 0.f, 2);
  }
  if (l2_regularize != 0.f) {  // (as many threads as the atomic form had: kFinishL2Parts blocks of 1024 where it had 1024 of 256)
    const int parts = grid_for((long long)yv.rows * yv.cols, 1024, kFinishL2Parts);
    hipLaunchKernelGGL(sumsq_parts_kernel, dim3(parts), dim3(1024), 0, s, yv, sp->l2_part);
    hipLaunchKernelGGL(sum_parts_kernel, dim3(1), dim3(64), 0, s, sp->l2_part, parts, b.l2sum);
  }
  hipLaunchKernelGGL(chain_finalize_kernel, dim3(1), dim3(64), 0, s, b.num_lp, b.den_lp, b.xent, l2_regularize != 0.f ? b.l2sum : nullptr,
                     B, T, sp->weight, l2_regularize, results);
  hipLaunchKernelGGL(chain_guard_kernel, dim3(grid_for((long long)dv.rows * dv.cols, 256)), dim3(256), 0, s, results, yv,
                     sp->weight * l2_regularize, dv, xdv);
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}
// ---- the objective alone (tdnnf_chain_objf, tdnnf_net_objective), on the objective-only workspace (chain_plan.h): the same recursion, the
// posterior pass with no derivative to write -- it then forms the xent objective only -- and the kernels that finish the objective
int chain_objf_num_recursion(const tdnnf_supervision *sp, const tdnnf_den_graph *g, const tdnnf_mat *y, void *ws, hipStream_t s) {
  return num_recursion(sp, y, chain_objf_bufs(g, sp->B, sp->T, ws), s);
}
// xent_output null: the xent objective is zero
int chain_objf_num_xent(const tdnnf_den_graph *g, const tdnnf_supervision *sp, const tdnnf_mat *y, const tdnnf_mat *xent_output, void *ws, hipStream_t s) {
  const ChainBufs b = chain_objf_bufs(g, sp->B, sp->T, ws);
  if (xent_output) return num_xent(sp, y, xent_output, 0.f, nullptr, b, s, false);
  TDNNF_HIP(hipMemsetAsync(b.xent, 0, sizeof(double) * sp->B, s));
  return TDNNF_OK;
}
int chain_objf_finish(const tdnnf_den_graph *g, const tdnnf_supervision *sp, const tdnnf_mat *y, float l2_regularize, double *results, void *ws, hipStream_t s) {
  const int B = sp->B, T = sp->T;
  const ChainBufs b = chain_objf_bufs(g, B, T, ws);
  if (l2_regularize != 0.f) {
    hipLaunchKernelGGL(sumsq_parts_kernel, dim3(kObjfL2Parts), dim3(1024), 0, s, view(y), b.l2part);
    hipLaunchKernelGGL(sum_parts_kernel, dim3(1), dim3(64), 0, s, b.l2part, kObjfL2Parts, b.l2sum);
  }
  hipLaunchKernelGGL(chain_finalize_kernel, dim3(1), dim3(64), 0, s, b.num_lp, b.den_lp, b.xent, l2_regularize != 0.f ? b.l2sum : nullptr, B, T, sp->weight,
                     l2_regularize, results);
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}
}  // namespace tdnnf

using namespace tdnnf;

extern "C" {

int tdnnf_chain_objf_and_deriv(const tdnnf_den_graph *g, const tdnnf_supervision *sp, const tdnnf_mat *y,
                               const tdnnf_mat *xent_output, float leaky, float l2_regularize, float xent_regularize,
                               double *results, tdnnf_mat *deriv, tdnnf_mat *xent_deriv, void *ws, size_t ws_bytes,
                               tdnnf_stream stream) {
  TDNNF_REQUIRE(g && sp && mat_ok(y) && mat_ok(deriv) && results, "chain_objf_and_deriv: bad arguments");
  if (int rc = sup_need_minibatch(sp, "chain_objf_and_deriv: ")) return rc;
  const int B = sp->B, T = sp->T;
  TDNNF_REQUIRE(y->rows == B * T && y->cols == g->P && same_dim(y, deriv), "chain_objf_and_deriv: nnet_output must be (B*T) x num_pdfs, t-major");
  TDNNF_REQUIRE(!xent_deriv || (mat_ok(xent_deriv) && same_dim(y, xent_deriv)), "chain_objf_and_deriv: bad xent_deriv");
  TDNNF_REQUIRE(!xent_output || (mat_ok(xent_output) && same_dim(y, xent_output)), "chain_objf_and_deriv: bad xent_output");
  TDNNF_REQUIRE(ws && ws_bytes >= tdnnf_chain_workspace_bytes(g, B, T), "chain_objf_and_deriv: workspace too small");
  TDNNF_REQUIRE(sp->kind == 0 || sp->num_pdfs <= g->P, "chain_objf_and_deriv: the supervision's num_pdfs %d exceeds the denominator graph's %d", sp->num_pdfs, g->P);
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if ((rc = chain_den(g, sp, y, leaky, deriv, ws, s))) return rc;
  if ((rc = chain_num(g, sp, y, xent_output, xent_regularize, xent_deriv, ws, s))) return rc;
  return chain_finish(g, sp, y, l2_regularize, results, deriv, xent_deriv, ws, s);
}

int tdnnf_chain_objf(const tdnnf_den_graph *g, const tdnnf_supervision *sp, const tdnnf_mat *y, const tdnnf_mat *xent_output, float leaky, float l2_regularize,
                     double *results, void *ws, size_t ws_bytes, tdnnf_stream stream) {
  TDNNF_REQUIRE(g && sp && mat_ok(y) && results, "chain_objf: bad arguments");
  if (int rc = sup_need_minibatch(sp, "chain_objf: ")) return rc;
  const int B = sp->B, T = sp->T;
  TDNNF_REQUIRE(y->rows == B * T && y->cols == g->P, "chain_objf: nnet_output must be (B*T) x num_pdfs, t-major");
  TDNNF_REQUIRE(!xent_output || (mat_ok(xent_output) && same_dim(y, xent_output)), "chain_objf: bad xent_output");
  TDNNF_REQUIRE(ws && ws_bytes >= tdnnf_chain_objf_workspace_bytes(g, B, T), "chain_objf: workspace too small");
  TDNNF_REQUIRE(sp->kind == 0 || sp->num_pdfs <= g->P, "chain_objf: the supervision's num_pdfs %d exceeds the denominator graph's %d", sp->num_pdfs, g->P);
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if ((rc = chain_objf_den(g, sp, y, leaky, ws, s))) return rc;
  if ((rc = num_recursion(sp, y, chain_objf_bufs(g, B, T, ws), s, !xent_output))) return rc;
  if ((rc = chain_objf_num_xent(g, sp, y, xent_output, ws, s))) return rc;
  return chain_objf_finish(g, sp, y, l2_regularize, results, ws, s);
}

int tdnnf_chain_numerator_part(const tdnnf_den_graph *g, const tdnnf_supervision *sp, const tdnnf_mat *y, int part, double *results, tdnnf_mat *deriv,
                               tdnnf_mat *xent_deriv, void *ws, size_t ws_bytes, tdnnf_stream stream) {
  TDNNF_REQUIRE(g && sp && mat_ok(y) && y->rows == sp->B * sp->T && y->cols == g->P, "chain_numerator_part: bad arguments");
  if (int rc = sup_need_minibatch(sp, "chain_numerator_part: ")) return rc;
  TDNNF_REQUIRE(ws && ws_bytes >= tdnnf_chain_workspace_bytes(g, sp->B, sp->T), "chain_numerator_part: workspace too small");
  TDNNF_REQUIRE(sp->kind == 0 || sp->num_pdfs <= g->P, "chain_numerator_part: the supervision's num_pdfs %d exceeds the denominator graph's %d", sp->num_pdfs, g->P);
  hipStream_t s = (hipStream_t)stream;
  if (part == 1) return chain_num_recursion(sp, g, y, ws, s);
  if (part == 4) {
    TDNNF_REQUIRE(mat_ok(xent_deriv) && same_dim(y, xent_deriv), "chain_numerator_part: part 4 needs xent_deriv");
    return chain_num_xent(g, sp, y, nullptr, 0.1f, xent_deriv, ws, s, true);
  }
  TDNNF_REQUIRE(part == 2 && results && mat_ok(deriv) && same_dim(y, deriv), "chain_numerator_part: part is 1, 4 or 2 (which needs results and nnet_output_deriv)");
  return chain_finish(g, sp, y, 0.f, results, deriv, nullptr, ws, s);
}

}  // extern "C"
