// num_e2e_kernels.h -- the chain numerator on cyclic per-sequence graphs (flat-start / "end-to-end" LF-MMI: Kaldi's
// GenericNumeratorComputation).  Included by chain_num_e2e.hip only.  The graphs are a tdnnf_align_graphs (align_graphs.h: the arcs by
// destination, by source and by pdf), one graph per sequence; the arithmetic is align_fb_kernels.h's with acoustic_scale = 1, all in double,
// and so is the code: its forward pass (fb_forward), its step on the arcs by source (align_step with AlignLseAcc) and its per-pdf sum (fb_post_step):
//     term(arc, t) = (double)arc_logprob + (double)y[t * B + s, arc_pdf]                        no clamp
//     alpha_0 = initial_logprob;  alpha_t+1[d] = LSE over arcs into d of alpha_t[src] + term(arc, t)
//     num_lp[s] = LSE over states of alpha_T + final_logprob
//     beta_T = final_logprob;     beta_t[st] = LSE over arcs out of st of term(arc, t) + beta_t+1[dst]
//     gamma[t, p] = sum over arcs with pdf p of exp(alpha_t[src] + term + beta_t+1[dst] - num_lp[s])
//
// Two kernels, where align_fb_kernel is one: that kernel forms row t of the posteriors inside its serial backward loop, which triples the
// time its workgroup holds the critical path (docs/experiments.md r6-p).  Here
//  * num_e2e_recursion_kernel: one workgroup per sequence, the alignment's schedule (thread counts, state vectors in LDS or in the
//    supervision's scratch, the next frame's output row staged one frame ahead), workgroup barriers only, every loop bounded by T.  It
//    keeps alpha_t and beta_t of EVERY frame in the supervision's scratch ((T + 1) * S doubles each) and needs the chain output only, so
//    the trainer starts it beside the denominator.  !FULL: the forward half alone on its two alternating vectors, nothing kept per frame.
//  * num_e2e_posterior_kernel: grid (ceil(T / kNumE2eFrames), B), alpha_t and beta_t+1 of the frame at hand staged in LDS where the
//    recursion's vectors live there.  A (frame, pdf) element has one owner -- a lane per pdf from the by-pdf
//    table's slices, a wave per pdf that more than kAlignHeavy arcs name -- which sums the pdf's arcs in the caller's order, recomputing
//    term: no atomics, nothing kept per arc, the same bits on every call.  It ADDS (float)(weight * gamma) into deriv (behind the
//    denominator's term) and / or xent_scale times it into xent_deriv, and forms the xent objective as one partial sum per workgroup,
//    which num_e2e_xent_sum_kernel adds in ascending order.  Elements whose pdf no arc of the sequence names are not touched.  A sequence
//    whose num_lp is not finite is skipped: the failure path of chain_finalize_kernel / chain_guard_kernel zeroes the matrices, and no
//    NaN is formed to be overwritten.
#pragma once
#include "align_fb_kernels.h"

namespace tdnnf {
namespace {

constexpr int kNumE2eFrames = 8;  // frames per workgroup of the posterior pass (the wide numerator's kNumWideFrames)

// grid = sequences; sequence s walks graph s.  Dynamic LDS: [LDS: 2 * Smax doubles, the state vectors] [YLDS: 2 * P floats, two output rows].
// alpha_all / beta_all: the (T + 1) * S doubles of the sequence whose first state is state0 start at (T + 1) * state0; vecs (!LDS): its two
// vectors at 2 * state0.
template <int NT, bool LDS, bool YLDS, bool FULL>
__global__ __launch_bounds__(NT) void num_e2e_recursion_kernel(AlignDev g, MatView y, int B, int T, double *alpha_all, double *beta_all, double *vecs,
                                                               double *num_lp, int Smax, int P) {
  static_assert(LDS || !YLDS, "the rows behind the vectors need the LDS form");
  extern __shared__ double num_e2e_smem[];
  const int tid = threadIdx.x, seq = blockIdx.x;
  const AlignGraphDev gr = g.graphs[seq];
  const int S = gr.num_states, s0 = gr.state0;
  double *cur = LDS ? num_e2e_smem : vecs + 2 * (size_t)s0, *nxt = cur + S;
  // t-major: the next frame's row of this sequence lies B rows on
  AlignRowStage<NT, YLDS> rows(y.data + (size_t)seq * y.stride, (size_t)B * y.stride, P, T, reinterpret_cast<float *>(num_e2e_smem + 2 * (size_t)Smax));
  const double logprob = fb_forward<NT, YLDS, FULL>(g, gr, T, rows, 1.0, cur, nxt, FULL ? alpha_all + (size_t)(T + 1) * s0 : nullptr);
  if (tid == 0) num_lp[seq] = logprob;
  if (!FULL) return;
  if (!(logprob > -INFINITY && logprob < INFINITY)) return;  // (the posterior pass skips this sequence: its beta has no reader)
  double *beta = beta_all + (size_t)(T + 1) * s0;
  // (alpha_T's last readers are behind the barrier above)
  for (int s = tid; s < S; s += NT) {
    const double v = (double)g.final[s0 + s];
    cur[s] = v;
    beta[(size_t)T * S + s] = v;
  }
  rows.load(T - 1);
  rows.store(T - 1);
  rows.load(T - 2);
  __syncthreads();
  for (int t = T - 1; t >= 0; t--) {
    // row t - 1 into the buffer whose last readers -- frame t + 1 -- are behind the previous barrier; row t - 2 on its way
    rows.store(t - 1);
    rows.load(t - 2);
    align_step<NT>(g.by_src, gr.by_src, cur, rows.row(t), 1.0, AlignLseAcc{nxt, beta + (size_t)t * S});
    __syncthreads();
    double *sw = cur;
    cur = nxt;
    nxt = sw;
  }
}

// grid (ceil(T / kNumE2eFrames), B).  deriv += (float)(weight * gamma), xent_deriv += xent_scale * that (either may be absent);
// do_xent: the workgroup's share of the xent objective -> xent_part[s * gridDim.x + block] (0 for a skipped sequence).
// LDS: alpha_t and beta_t+1 of the frame being worked on are staged in 2 * Smax doubles of dynamic LDS (coalesced loads, two barriers a
// frame) and the arcs gather from there: a gather of 8 bytes from global memory moves a whole cache line, and on a 4 000-state graph those
// lines were the pass's time (20.2 ms a pass at 128 x 150 frames against 12.0 ms for all of align_fb_kernel; docs/experiments.md r6-q).
// NT: 256 threads, 1024 where the largest graph has more than 1024 states (two such workgroups still fit a CU beside their vectors).
template <int NT, bool LDS>
__global__ __launch_bounds__(NT) void num_e2e_posterior_kernel(AlignDev g, MatView y, MatView xent_out, int B, int T, float weight, const double *alpha_all,
                                                               const double *beta_all, const double *num_lp, MatView deriv, MatView xent_deriv,
                                                               float xent_scale, int do_xent, double *xent_part, int Smax) {
  extern __shared__ double num_e2e_post_smem[];
  __shared__ double red[NT / 64];
  const int seq = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double logprob = num_lp[seq], w = (double)weight;
  double xo = 0.0;
  auto emit = [&](size_t row, int pdf, double sum) {
    const float gam = (float)(w * sum);
    if (deriv.data) deriv.data[row * deriv.stride + pdf] += gam;
    if (xent_deriv.data) xent_deriv.data[row * xent_deriv.stride + pdf] += xent_scale * gam;
    if (do_xent && xent_out.data) xo += (double)gam * (double)xent_out.data[row * xent_out.stride + pdf];
  };
  if (logprob > -INFINITY && logprob < INFINITY) {  // (the same for every thread of the workgroup: the barriers below are met by all or none)
    const AlignGraphDev gr = g.graphs[seq];
    const int S = gr.num_states, t0 = blockIdx.x * kNumE2eFrames, t1 = min(T, t0 + kNumE2eFrames);
    const double *alpha = alpha_all + (size_t)(T + 1) * gr.state0, *beta = beta_all + (size_t)(T + 1) * gr.state0;
    for (int t = t0; t < t1; t++) {
      const double *at = alpha + (size_t)t * S, *bt = beta + (size_t)(t + 1) * S;
      if (LDS) {
        double *al = num_e2e_post_smem, *bl = al + Smax;
        if (t > t0) __syncthreads();  // the last frame's readers are done
        for (int s = tid; s < S; s += NT) {
          al[s] = at[s];
          bl[s] = bt[s];
        }
        __syncthreads();
        at = al;
        bt = bl;
      }
      const size_t row = (size_t)t * B + seq;
      fb_post_step<NT>(g.by_pdf, gr.by_pdf, at, bt, y.data + row * y.stride, 1.0, logprob, [&](int pdf, int, double sum) { emit(row, pdf, sum); });
    }
  }
  if (do_xent) {
    for (int o = 32; o > 0; o >>= 1) xo += __shfl_xor(xo, o, 64);
    if (lane == 0) red[wave] = xo;
    __syncthreads();
    if (tid == 0) {
      double x = 0.0;
      for (int k = 0; k < NT / 64; k++) x += red[k];
      xent_part[(size_t)seq * gridDim.x + blockIdx.x] = x;
    }
  }
}

// xent_objf[s] = the sum of sequence s's partial sums, in ascending order
__global__ void num_e2e_xent_sum_kernel(const double *part, int B, int blocks, double *xent_objf) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= B) return;
  double x = 0.0;
  for (int k = 0; k < blocks; k++) x += part[(size_t)s * blocks + k];
  xent_objf[s] = x;
}

}  // namespace
}  // namespace tdnnf
