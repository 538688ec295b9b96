// num_wide_kernels.h -- the chain numerator for supervisions of any width (lattices with a frame tolerance: tens to hundreds of states per
// frame).  Included by chain_num.hip behind log_add; numerator_kernel there stays what narrow supervisions run.
//
//  * recursion: one workgroup per sequence.  The log alpha (then log beta) of the frame being read and of the frame being written live in LDS,
//    ping-pong; so do the frame's arc scores lp + y[t, pdf] and source indexes, which do not depend on the recursion: a register pipeline loads
//    the arcs two frames ahead and gathers their y one frame ahead, so that what a frame waits for behind its barrier is LDS only
//    (read, log_add, write).  Same arithmetic in the same arc order as numerator_kernel: la / lb come out equal bit for bit.
//  * posteriors: workgroups over (sequence, block of kNumWideFrames frames), threads over the block's arcs, which the supervision holds
//    ordered by (frame, pdf): the first thread of a run of equal (frame, pdf) sums the run in order and adds it to the output once.  A row
//    belongs to one workgroup, there are no atomics, the result is reproducible bit for bit.
#pragma once
#include "chain_types.h"

namespace tdnnf {
namespace {

constexpr int kNumWideArcRegs = 4;  // arcs of a frame per thread that the register pipeline carries (the rest are staged behind the frame's work)

// dynamic LDS of num_wide_recursion_kernel: [4 doubles of the reduction] [2 frontiers of W doubles] [2 x A arc scores] [2 x A source indexes]
// [frame_state_begin, first in-arc, first out-arc of every frame: 3 x (T + 2) ints]
inline size_t num_wide_lds(int W, int A, int T) { return 8 * (4 + 2 * (size_t)W + 2 * (size_t)A) + 4 * (2 * (size_t)A + 3 * (size_t)(T + 2)); }

// One direction of the recursion.  Step i computes frame f(i) from frame p(i) with output row r(i): forward f = i + 1, p = r = i over the arcs
// grouped by destination; backward f = r = T - 1 - i, p = T - i over the arcs grouped by source.  fr + cur * W holds frame p(0) on entry.
// Returns the buffer that holds the last frame computed.
template <int NT, bool FWD>
__device__ __forceinline__ int num_wide_pass(const int *begin, const int *other, const int *pdfs, const float *lps, const MatView &y, int B, int T, int s,
                                             const int *fsb, const int *ab, double *fr, int W, double *ssc, int *sso, int A, int cur, double *out) {
  constexpr int R = kNumWideArcRegs;
  const int tid = threadIdx.x;
  struct Regs {
    int pdf[R], oth[R], b0, b1;
    float lp[R];
  };
  auto frame = [&](int i) { return FWD ? i + 1 : T - 1 - i; };
  auto prev = [&](int i) { return FWD ? i : T - i; };
  // the arcs of step i (R per thread) and the arc range of the thread's first state
  auto load_arcs = [&](int i, Regs &q) {
    if (i >= T) return;
    const int f = frame(i), a0 = ab[f], a1 = ab[f + 1], p0 = fsb[prev(i)];
#pragma unroll
    for (int r = 0; r < R; r++) {
      const int a = a0 + tid + r * NT;
      if (a < a1) {
        q.pdf[r] = pdfs[a];
        q.oth[r] = other[a] - p0;
        q.lp[r] = lps[a];
      }
    }
    const int st = fsb[f] + tid;
    if (st < fsb[f + 1]) {
      q.b0 = begin[st] - a0;
      q.b1 = begin[st + 1] - a0;
    }
  };
  auto gather_y = [&](int i, const Regs &q, float (&yv)[R]) {
    if (i >= T) return;
    const int f = frame(i), n = ab[f + 1] - ab[f];
    const float *yrow = y.data + (size_t)((FWD ? i : f) * B + s) * y.stride;
#pragma unroll
    for (int r = 0; r < R; r++)
      if (tid + r * NT < n) yv[r] = yrow[q.pdf[r]];
  };
  // scores and source indexes of step i into its LDS buffer (arcs beyond the pipeline's R * NT: loaded here)
  auto stage = [&](int i, const Regs &q, const float (&yv)[R]) {
    if (i >= T) return;
    const int f = frame(i), a0 = ab[f], n = ab[f + 1] - a0, p0 = fsb[prev(i)];
    double *sc = ssc + (size_t)(i & 1) * A;
    int *so = sso + (size_t)(i & 1) * A;
#pragma unroll
    for (int r = 0; r < R; r++) {
      const int j = tid + r * NT;
      if (j < n) {
        sc[j] = (double)q.lp[r] + (double)yv[r];
        so[j] = q.oth[r];
      }
    }
    const float *yrow = y.data + (size_t)((FWD ? i : f) * B + s) * y.stride;
    for (int j = tid + R * NT; j < n; j += NT) {
      sc[j] = (double)lps[a0 + j] + (double)yrow[pdfs[a0 + j]];
      so[j] = other[a0 + j] - p0;
    }
  };
  Regs q1 = {}, q2 = {};
  float yv[R] = {};
  load_arcs(0, q1);
  gather_y(0, q1, yv);
  stage(0, q1, yv);
  int cb0 = q1.b0, cb1 = q1.b1;
  load_arcs(1, q1);
  __syncthreads();
  for (int i = 0; i < T; i++) {
    gather_y(i + 1, q1, yv);  // (its pdfs were loaded one step ago)
    load_arcs(i + 2, q2);
    {  // frame f(i): LDS only for a thread's first state (frames wider than the workgroup: further states read their arc range from memory)
      const int f = frame(i), f0 = fsb[f], n = fsb[f + 1] - f0, a0 = ab[f];
      const double *frc = fr + (size_t)cur * W, *sc = ssc + (size_t)(i & 1) * A;
      const int *so = sso + (size_t)(i & 1) * A;
      double *frn = fr + (size_t)(cur ^ 1) * W;
      for (int k = tid; k < n; k += NT) {
        const int b0 = k == tid ? cb0 : begin[f0 + k] - a0, b1 = k == tid ? cb1 : begin[f0 + k + 1] - a0;
        double v = -INFINITY;
        for (int j = b0; j < b1; j++) v = log_add(v, frc[so[j]] + sc[j]);
        frn[k] = v;
        out[f0 + k] = v;
      }
    }
    stage(i + 1, q1, yv);
    cb0 = q1.b0;
    cb1 = q1.b1;
    q1 = q2;
    cur ^= 1;
    __syncthreads();
  }
  return cur;
}

// total of a sequence from its threads' partial log-sums: the wave's butterfly (as numerator_kernel), then the waves in order
template <int NT>
__device__ __forceinline__ double num_wide_total(double tot, double *red) {
  for (int o = 32; o > 0; o >>= 1) tot = log_add(tot, __shfl_xor(tot, o, 64));
  if (NT == 64) return tot;
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = tot;
  __syncthreads();
  tot = red[0];
  for (int w = 1; w < NT / 64; w++) tot = log_add(tot, red[w]);
  return tot;
}

template <int NT>
__global__ __launch_bounds__(NT) void num_wide_recursion_kernel(SupDev sp, MatView y, double *la, double *lb, double *num_logprob, int W, int A) {
  extern __shared__ double num_wide_smem[];
  const int s = blockIdx.x, tid = threadIdx.x, B = sp.B, T = sp.T;
  double *red = num_wide_smem, *fr = red + 4, *ssc = fr + 2 * (size_t)W;
  int *sso = reinterpret_cast<int *>(ssc + 2 * (size_t)A), *fsb = sso + 2 * (size_t)A, *abi = fsb + (T + 2), *abo = abi + (T + 2);
  const int *gfsb = sp.frame_state_begin + (size_t)s * (T + 2);
  for (int t = tid; t < T + 2; t += NT) {
    const int f = gfsb[t];
    fsb[t] = f;
    abi[t] = sp.in_begin[f];
    abo[t] = sp.out_begin[f];
  }
  if (tid == 0) {
    fr[0] = 0.0;
    la[gfsb[0]] = 0.0;
  }
  __syncthreads();
  int cur = num_wide_pass<NT, true>(sp.in_begin, sp.in_src, sp.in_pdf, sp.in_lp, y, B, T, s, fsb, abi, fr, W, ssc, sso, A, 0, la);
  // frame T: log beta = the final log-prob, total = log sum of alpha + final
  const int fT = fsb[T], nT = fsb[T + 1] - fT;
  const double *frc = fr + (size_t)cur * W;
  double *frn = fr + (size_t)(cur ^ 1) * W;
  double tot = -INFINITY;
  for (int k = tid; k < nT; k += NT) {
    const float f = sp.final_logprob[fT + k];
    lb[fT + k] = (double)f;
    frn[k] = (double)f;
    if (f != -INFINITY) tot = log_add(tot, frc[k] + (double)f);
  }
  tot = num_wide_total<NT>(tot, red);
  if (tid == 0) num_logprob[s] = tot;
  __syncthreads();
  num_wide_pass<NT, false>(sp.out_begin, sp.out_dst, sp.out_pdf, sp.out_lp, y, B, T, s, fsb, abo, fr, W, ssc, sso, A, cur ^ 1, lb);
}

// the same recursion with the frontier in global memory (la / lb themselves), for a supervision whose widest frame does not fit the LDS
template <int NT>
__global__ __launch_bounds__(NT) void num_wide_recursion_global_kernel(SupDev sp, MatView y, double *la, double *lb, double *num_logprob) {
  __shared__ double red[4];
  const int s = blockIdx.x, tid = threadIdx.x, B = sp.B, T = sp.T;
  const int *fsb = sp.frame_state_begin + (size_t)s * (T + 2);
  if (tid == 0) la[fsb[0]] = 0.0;
  __syncthreads();
  for (int t = 1; t <= T; t++) {
    const float *yrow = y.data + (size_t)((t - 1) * B + s) * y.stride;
    for (int st = fsb[t] + tid; st < fsb[t + 1]; st += NT) {
      double v = -INFINITY;
      for (int a = sp.in_begin[st]; a < sp.in_begin[st + 1]; a++) v = log_add(v, la[sp.in_src[a]] + ((double)sp.in_lp[a] + (double)yrow[sp.in_pdf[a]]));
      la[st] = v;
    }
    __syncthreads();
  }
  double tot = -INFINITY;
  for (int st = fsb[T] + tid; st < fsb[T + 1]; st += NT) {
    const float f = sp.final_logprob[st];
    lb[st] = (double)f;
    if (f != -INFINITY) tot = log_add(tot, la[st] + (double)f);
  }
  tot = num_wide_total<NT>(tot, red);
  if (tid == 0) num_logprob[s] = tot;
  __syncthreads();
  for (int t = T - 1; t >= 0; t--) {
    const float *yrow = y.data + (size_t)(t * B + s) * y.stride;
    for (int st = fsb[t] + tid; st < fsb[t + 1]; st += NT) {
      double v = -INFINITY;
      for (int a = sp.out_begin[st]; a < sp.out_begin[st + 1]; a++) v = log_add(v, ((double)sp.out_lp[a] + (double)yrow[sp.out_pdf[a]]) + lb[sp.out_dst[a]]);
      lb[st] = v;
    }
    __syncthreads();
  }
}

constexpr int kNumWidePostThreads = 256;

// grid (ceil(T / kNumWideFrames), B).  deriv += weight * gamma, xent_deriv += xent_scale * weight * gamma (either may be absent);
// do_xent: the block's share of the xent objective -> w.xent_part[s * gridDim.x + block]
__global__ __launch_bounds__(kNumWidePostThreads) void num_wide_posterior_kernel(SupDev sp, SupWideDev w, MatView y, MatView xent_out, const double *la,
                                                                                 const double *lb, const double *num_logprob, MatView deriv,
                                                                                 MatView xent_deriv, float xent_scale, int do_xent) {
  constexpr int NT = kNumWidePostThreads;
  __shared__ float g[NT];
  __shared__ int kt[NT], kp[NT];
  __shared__ double red[NT / 64];
  const int s = blockIdx.y, tid = threadIdx.x, B = sp.B, T = sp.T;
  const int *fsb = sp.frame_state_begin + (size_t)s * (T + 2);
  const int t0 = blockIdx.x * kNumWideFrames, t1 = min(T, t0 + kNumWideFrames);
  const int a0 = sp.out_begin[fsb[t0]], a1 = sp.out_begin[fsb[t1]];
  const double tot = num_logprob[s];
  double xo = 0.0;
  for (int base = a0; base < a1; base += NT) {
    const int a = base + tid;
    const bool valid = a < a1;
    int t = -1, pdf = -1;
    float gam = 0.f;
    size_t row = 0;
    if (valid) {
      t = w.pf_t[a];
      pdf = w.pf_pdf[a];
      row = (size_t)(t * B + s);
      const double ll = (double)w.pf_lp[a] + (double)y.data[row * y.stride + pdf];
      gam = sp.weight * (float)exp(la[w.pf_src[a]] + ll + lb[w.pf_dst[a]] - tot);
      if (do_xent && xent_out.data) xo += (double)gam * (double)xent_out.data[row * xent_out.stride + pdf];
    }
    g[tid] = gam;
    kt[tid] = t;
    kp[tid] = pdf;
    __syncthreads();
    if (valid && (tid == 0 || kt[tid - 1] != t || kp[tid - 1] != pdf)) {  // the first arc of a run of one (frame, pdf): the run's sum, added once
      float sum = gam;
      for (int j = tid + 1; j < NT && kt[j] == t && kp[j] == pdf; j++) sum += g[j];
      if (deriv.data) deriv.data[row * deriv.stride + pdf] += sum;
      if (xent_deriv.data) xent_deriv.data[row * xent_deriv.stride + pdf] += xent_scale * sum;
    }
    __syncthreads();  // (a run that crosses into the next NT arcs is added to twice, by this workgroup, one after the other)
  }
  if (do_xent) {
    for (int o = 32; o > 0; o >>= 1) xo += __shfl_xor(xo, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = xo;
    __syncthreads();
    if (tid == 0) w.xent_part[(size_t)s * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

__global__ void num_wide_xent_sum_kernel(const double *part, int B, int blocks, double *xent_objf) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= B) return;
  double x = 0.0;
  for (int k = 0; k < blocks; k++) x += part[(size_t)s * blocks + k];
  xent_objf[s] = x;
}

}  // namespace
}  // namespace tdnnf
