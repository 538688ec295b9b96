// align_fb_kernels.h -- forward-backward through the graphs of align_kernels.h: total log-likelihood (log-sum over all paths) and per-frame
// pdf posteriors.  Included by align_fb.hip only.
//
// Arithmetic (include/tdnnf_hip.h, "forward-backward"; held to a tolerance by tests/test_gpu_posteriors.py against tests/posteriors_ref64.py):
//     term(arc, t) = (double)arc_logprob + (double)acoustic_scale * (double)y[t, arc_pdf]          (align_kernels.h's, rounded once either way)
//     alpha_0[s]   = (double)initial_logprob[s]
//     alpha_t+1[d] = LSE over arcs into d   of  alpha_t[src] + term(arc, t)
//     logprob      = LSE over s             of  alpha_T[s] + (double)final_logprob[s]
//     beta_T[s]    = (double)final_logprob[s]
//     beta_t[s]    = LSE over arcs out of s of  term(arc, t) + beta_t+1[dst]
//     gamma[t, p]  = sum over arcs with pdf p of exp(alpha_t[src] + term(arc, t) + beta_t+1[dst] - logprob)
//     post[t, p]   = (float)(weight * gamma[t, p])
//   LSE keeps a running (m, sum): m the greatest candidate so far, sum = sum of exp(candidate - m), rescaled when m grows -- ONE exp per
//   candidate (exp(-|candidate - m|) serves both cases) and one pass over a row; the result is m + log(sum), -inf for no candidate, +inf
//   when a candidate is +inf.  A candidate counts only if it compares greater than -inf: a NaN or -inf one adds nothing and a NaN never
//   enters a state vector.  exp and log are the device library's double functions; contraction is off in the helpers, so every launch form
//   rounds alike.
//
// One workgroup per utterance, the alignment's schedule: forward over the arcs by destination (the alignment's own table and loop shape,
// a log-sum where it takes a max), the total, then -- with a posterior matrix and a finite total -- backward from frame T - 1 to 0:
//   1. beta_t from the arcs by source (the same loop on another table: term + beta_t+1[dst] is the same sum as alpha_t[src] + term);
//   2. row t of post from the arcs by pdf: a lane per pdf (a wave per pdf named by more than kAlignHeavy arcs), the arcs in the caller's
//      order, so every element has one owner and one order of summation.  The row is first zeroed by coalesced stores, and behind the
//      barrier that separates step 1 from step 2 the owners store their elements straight to global memory: no LDS row of num_pdfs
//      floats, no atomics.  Step 2 recomputes term + beta_t+1[dst] per arc; step 1 leaves nothing per arc.
// alpha_t of every frame is kept in the workspace ((T + 1) * S doubles) by the forward pass when posteriors are wanted; without them the
// forward pass runs alone on its two alternating vectors.
//  * LDS: the two state vectors are 2 * Smax doubles of dynamic LDS, else they lie in the workspace;
//  * ALDS (LDS, posteriors): a third vector holds alpha_t: loaded from the workspace into kAlignFbAlphaRegs registers before step 1, stored
//    to LDS behind it, so the loads' latency hides behind step 1; else step 2 gathers alpha_t from the workspace;
//  * YLDS: two output rows behind the vectors, staged one frame ahead through registers as align_kernels.h does (backward: one frame behind).
#pragma once
#include "align_graphs.h"

namespace tdnnf {
namespace {

constexpr int kAlignFbAlphaRegs = 7;  // doubles of alpha_t a thread carries into LDS (ALDS): 7 * 1024 covers every S whose three vectors fit

struct AlignFbUtt {  // one utterance of a call (device table at the head of the workspace)
  int graph, frames;
  int row_begin, pad;
  long long alpha_begin;  // first double of its (frames + 1) * S alphas in the workspace's alpha region (posteriors)
  long long vec_begin;    // first double of its two state vectors in the workspace's vector region (workspace form)
};

static_assert(sizeof(AlignFbUtt) == 32, "the workspace formula of include/tdnnf_hip.h counts 32 bytes an utterance");

struct AlignFbDev {
  const AlignFbGraphDev *graphs;
  AlignFbTable by_src;  // rows: states; arcs (destination state LOCAL to its graph, pdf, log-prob bits, caller's arc index)
  AlignFbTable by_pdf;  // rows: pdfs;   arcs (source state, destination state, both LOCAL, log-prob bits, caller's arc index -- in .w)
};

// running log-sum: (m, s) takes candidate v
__device__ __forceinline__ void fb_lse_add(double &m, double &s, double v) {
#pragma clang fp contract(off)
  const double d = v - m;  // (m = -inf: +inf; both +inf: NaN, which only reaches s, and s is not read once m is +inf)
  const double e = exp(-fabs(d));
  const bool up = d > 0.0;
  const double s2 = up ? s * e + 1.0 : s + e;
  if (v > -INFINITY) {
    s = s2;
    m = up ? v : m;
  }
}
// (m, s) takes the partial result (om, os)
__device__ __forceinline__ void fb_lse_merge(double &m, double &s, double om, double os) {
#pragma clang fp contract(off)
  if (!(om > -INFINITY)) return;
  if (!(m > -INFINITY)) {
    m = om;
    s = os;
    return;
  }
  const double M = om > m ? om : m;
  if (M < INFINITY) s = s * exp(m - M) + os * exp(om - M);
  m = M;
}
__device__ __forceinline__ double fb_lse_value(double m, double s) { return (m > -INFINITY && m < INFINITY) ? m + log(s) : m; }
__device__ __forceinline__ void fb_lse_wave(double &m, double &s) {
  for (int o = 32; o > 0; o >>= 1) {
    const double om = __shfl_xor(m, o, 64);
    const double os = __shfl_xor(s, o, 64);
    fb_lse_merge(m, s, om, os);
  }
}

// One frame of a recursion on one table: out[row] = LSE over the row's arcs of from[arc.x] + term(arc).  Forward: the arcs by destination,
// arc.x the source; backward: the arcs by source, arc.x the destination.  keep (may be null): a second copy of the results.
template <int NT>
__device__ __forceinline__ void fb_lse_step(const int4 *slots, int num_slots, const int4 *heavy, int num_heavy, const int4 *arcs, const double *from,
                                            const float *yrow, double scale, double *out, double *keep, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  for (int slot = tid; slot < num_slots; slot += NT) {  // light rows: a lane per row, slice by slice
    const int4 row = slots[slot];
    if (row.x < 0) continue;
    double m = -INFINITY, s = 0.0;
    for (int j = 0; j < row.y; j += kAlignBatch) {
      int4 arc[kAlignBatch];
      float yv[kAlignBatch];
#pragma unroll
      for (int k = 0; k < kAlignBatch; k++) arc[k] = arcs[row.z + 64 * min(j + k, row.y - 1)];
#pragma unroll
      for (int k = 0; k < kAlignBatch; k++) yv[k] = yrow[arc[k].y];
#pragma unroll
      for (int k = 0; k < kAlignBatch; k++) {
        const double v = from[arc[k].x] + ((double)__int_as_float(arc[k].z) + scale * (double)yv[k]);
        // (no branch around the exp of a batch's padding: skipping it where a whole wave is past its rows' ends measured 1 % faster on
        // the 4 000-state graph and 11 % slower on transcript graphs, whose slices mix lengths: docs/experiments.md r6-p)
        fb_lse_add(m, s, j + k < row.y ? v : -INFINITY);
      }
    }
    const double r = fb_lse_value(m, s);
    out[row.x] = r;
    if (keep) keep[row.x] = r;
  }
  for (int h = wave; h < num_heavy; h += NT / 64) {  // heavy rows: a wave per row, the lanes' (m, s) merged by butterfly
    const int4 row = heavy[h];
    double m = -INFINITY, s = 0.0;
    for (int a = row.y + lane; a < row.z; a += 64) {
      const int4 arc = arcs[a];
      fb_lse_add(m, s, from[arc.x] + ((double)__int_as_float(arc.z) + scale * (double)yrow[arc.y]));
    }
    fb_lse_wave(m, s);
    if (lane == 0) {
      const double r = fb_lse_value(m, s);
      out[row.x] = r;
      if (keep) keep[row.x] = r;
    }
  }
}

// Row t of the posteriors from the arcs by pdf: prow[p] = (float)(weight * sum over the arcs of pdf p of exp(alpha[src] + term + beta[dst] - logprob)).
// Only the pdfs that an arc names have a row; the others keep the zero the caller stored.
template <int NT>
__device__ __forceinline__ void fb_post_step(const int4 *slots, int num_slots, const int4 *heavy, int num_heavy, const int4 *arcs, const double *alpha,
                                             const double *beta, const float *yrow, double scale, double logprob, double weight, float *prow, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  for (int slot = tid; slot < num_slots; slot += NT) {
    const int4 row = slots[slot];
    if (row.x < 0) continue;
    const double ay = scale * (double)yrow[row.x];
    double sum = 0.0;
    for (int j = 0; j < row.y; j += kAlignBatch) {
      int4 arc[kAlignBatch];
#pragma unroll
      for (int k = 0; k < kAlignBatch; k++) arc[k] = arcs[row.z + 64 * min(j + k, row.y - 1)];
#pragma unroll
      for (int k = 0; k < kAlignBatch; k++) {
        const double v = (alpha[arc[k].x] + ((double)__int_as_float(arc[k].z) + ay)) + beta[arc[k].y];
        if (j + k < row.y && v > -INFINITY) sum += exp(v - logprob);
      }
    }
    prow[row.x] = (float)(weight * sum);
  }
  for (int h = wave; h < num_heavy; h += NT / 64) {
    const int4 row = heavy[h];
    const double ay = scale * (double)yrow[row.x];
    double sum = 0.0;
    for (int a = row.y + lane; a < row.z; a += 64) {
      const int4 arc = arcs[a];
      const double v = (alpha[arc.x] + ((double)__int_as_float(arc.z) + ay)) + beta[arc.y];
      if (v > -INFINITY) sum += exp(v - logprob);
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) prow[row.x] = (float)(weight * sum);
  }
}

// grid = utterances.  Dynamic LDS: [LDS: 2 * Smax doubles, the state vectors] [ALDS: Smax doubles, alpha_t] [YLDS: 2 * P floats, two output rows].
// POST: alpha_all / post are read and written; otherwise the kernel ends with the total.
template <int NT, bool LDS, bool YLDS, bool ALDS, bool POST>
__global__ __launch_bounds__(NT) void align_fb_kernel(AlignDev g, AlignFbDev fb, const AlignFbUtt *utts, MatView y, int row_stride, float acoustic_scale,
                                                      float weight, MatView post, double *alpha_all, double *vecs, double *results, int Smax, int P) {
  static_assert(LDS || !(YLDS || ALDS), "the rows behind the vectors need the LDS form");
  static_assert(POST || !ALDS, "alpha_t is staged for the posteriors only");
  extern __shared__ double fb_smem[];
  __shared__ double red_m[NT / 64], red_s[NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const AlignFbUtt u = utts[blockIdx.x];
  const AlignGraphDev gr = g.graphs[u.graph];
  const int S = gr.num_states, T = u.frames, s0 = gr.state0;
  double *cur = LDS ? fb_smem : vecs + u.vec_begin, *nxt = cur + S;
  double *alds = fb_smem + 2 * (size_t)Smax;                                        // ALDS: alpha_t
  float *ylds = reinterpret_cast<float *>(fb_smem + (ALDS ? 3 : 2) * (size_t)Smax);  // YLDS: two rows of P floats
  double *alpha = POST ? alpha_all + u.alpha_begin : nullptr;
  const double scale = (double)acoustic_scale;
  float yreg[kAlignRowRegs];
  auto row_of = [&](int t) { return y.data + (size_t)(u.row_begin + (long long)t * row_stride) * y.stride; };
  auto load_row = [&](int t) {  // (only [0, P) of a row: what the graphs' arcs can name)
    if (!YLDS || t < 0 || t >= T) return;
    const float *r = row_of(t);
#pragma unroll
    for (int c = 0; c < kAlignRowRegs; c++)
      if (tid + c * NT < P) yreg[c] = r[tid + c * NT];
  };
  auto store_row = [&](int t) {
    if (!YLDS || t < 0 || t >= T) return;
#pragma unroll
    for (int c = 0; c < kAlignRowRegs; c++)
      if (tid + c * NT < P) ylds[(size_t)(t & 1) * P + tid + c * NT] = yreg[c];
  };
  for (int s = tid; s < S; s += NT) {
    const double v = (double)g.init[s0 + s];
    cur[s] = v;
    if (POST) alpha[s] = v;
  }
  load_row(0);
  store_row(0);
  load_row(1);
  __syncthreads();
  for (int t = 0; t < T; t++) {
    // row t + 1 (loaded a frame ago) into the buffer whose last readers -- frame t - 1 -- are behind the previous barrier; row t + 2 on its way
    store_row(t + 1);
    load_row(t + 2);
    const float *yrow = YLDS ? ylds + (size_t)(t & 1) * P : row_of(t);
    fb_lse_step<NT>(g.slots + gr.slot0, gr.num_slots, g.heavy + gr.heavy0, gr.num_heavy, g.arcs, cur, yrow, scale, nxt,
                    POST ? alpha + (size_t)(t + 1) * S : nullptr, tid);
    __syncthreads();
    double *sw = cur;
    cur = nxt;
    nxt = sw;
  }
  // the total: a thread's states in ascending order, the lanes by butterfly, the waves in ascending order -- by every thread alike
  double m = -INFINITY, sum = 0.0;
  for (int s = tid; s < S; s += NT) fb_lse_add(m, sum, cur[s] + (double)g.final[s0 + s]);
  fb_lse_wave(m, sum);
  if (lane == 0) {
    red_m[wave] = m;
    red_s[wave] = sum;
  }
  __syncthreads();
  m = red_m[0];
  sum = red_s[0];
  for (int w = 1; w < NT / 64; w++) fb_lse_merge(m, sum, red_m[w], red_s[w]);
  const double logprob = fb_lse_value(m, sum);
  const bool ok = logprob > -INFINITY && logprob < INFINITY;
  if (tid == 0) {
    results[2 * (size_t)blockIdx.x] = logprob;
    results[2 * (size_t)blockIdx.x + 1] = ok ? 1.0 : 0.0;
  }
  if (!POST) return;
  auto post_row = [&](int t) { return post.data + (size_t)(u.row_begin + (long long)t * row_stride) * post.stride; };
  if (!ok) {
    for (int t = 0; t < T; t++) {
      float *prow = post_row(t);
      for (int c = tid; c < P; c += NT) prow[c] = 0.f;
    }
    return;
  }
  const AlignFbGraphDev fg = fb.graphs[u.graph];
  const double w = (double)weight;
  // (alpha_T's last readers are behind the barrier above)
  for (int s = tid; s < S; s += NT) cur[s] = (double)g.final[s0 + s];
  load_row(T - 1);
  store_row(T - 1);
  load_row(T - 2);
  __syncthreads();
  for (int t = T - 1; t >= 0; t--) {
    // row t - 1 into the buffer whose last readers -- frame t + 1 -- are behind the previous barrier; row t - 2 on its way
    store_row(t - 1);
    load_row(t - 2);
    const float *yrow = YLDS ? ylds + (size_t)(t & 1) * P : row_of(t);
    float *prow = post_row(t);
    for (int c = tid; c < P; c += NT) prow[c] = 0.f;
    const double *at = alpha + (size_t)t * S;
    double areg[kAlignFbAlphaRegs];
    if (ALDS) {
#pragma unroll
      for (int c = 0; c < kAlignFbAlphaRegs; c++)
        if (tid + c * NT < S) areg[c] = at[tid + c * NT];
    }
    if (t > 0)  // (beta_0 has no reader)
      fb_lse_step<NT>(fb.by_src.slots + fg.src_slot0, fg.src_num_slots, fb.by_src.heavy + fg.src_heavy0, fg.src_num_heavy, fb.by_src.arcs, cur, yrow, scale,
                      nxt, nullptr, tid);
    if (ALDS) {
#pragma unroll
      for (int c = 0; c < kAlignFbAlphaRegs; c++)
        if (tid + c * NT < S) alds[tid + c * NT] = areg[c];
    }
    __syncthreads();  // alpha_t is in place and the row's zeros are stored
    fb_post_step<NT>(fb.by_pdf.slots + fg.pdf_slot0, fg.pdf_num_slots, fb.by_pdf.heavy + fg.pdf_heavy0, fg.pdf_num_heavy, fb.by_pdf.arcs,
                     ALDS ? (const double *)alds : at, cur, yrow, scale, logprob, w, prow, tid);
    __syncthreads();
    double *sw = cur;
    cur = nxt;
    nxt = sw;
  }
}

}  // namespace
}  // namespace tdnnf
