// align_fb_kernels.h -- forward-backward through the graphs of align_graphs.h: total log-likelihood (log-sum over all paths) and per-frame
// pdf (or label) posteriors.  Included by align_fb.hip and, for the shared parts (AlignLseAcc, fb_forward, fb_post_step), by num_e2e_kernels.h.
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
// One workgroup per utterance, the alignment's schedule: forward over the arcs by destination (the alignment's own table and step, align_step,
// with a log-sum accumulator where it takes a max), the total, then -- with a posterior matrix and a finite total -- backward from frame T - 1 to 0:
//   1. beta_t from the arcs by source (the same loop on another table: term + beta_t+1[dst] is the same sum as alpha_t[src] + term);
//   2. row t of post from the arcs by pdf: a lane per pdf (a wave per pdf named by more than kAlignHeavy arcs), the arcs in the caller's
//      order, so every element has one owner and one order of summation.  The row is first zeroed by coalesced stores, and behind the
//      barrier that separates step 1 from step 2 the owners store their elements straight to global memory: no LDS row of num_pdfs
//      floats, no atomics.  Step 2 recomputes term + beta_t+1[dst] per arc; step 1 leaves nothing per arc.
//      The COMPACT form (align_fb_compact_kernel, FbCompactOut) runs the same steps, but an utterance's output is frames x D floats, D the
//      distinct pdfs of its graph, and the owner of pdf p stores to the column of p (its rank among them, which comes with the by-pdf
//      row): every column of a frame has an owner, so there is no zeroing loop in the frame, and the values are the dense form's bits.
//      The LABEL form (align_fb_label_kernel, FbLabelStep) is the compact form on the fourth table: step 2 walks the arcs by LABEL (the
//      caller's second integer per arc: a transition-id, a phone, the arc's index) with fb_label_step, the same row walk, which reads
//      y[t, pdf of the arc] per arc where fb_post_step reads y[t, pdf of the row] once; the output is frames x L floats, L the distinct
//      labels of the graph.  With label = pdf both steps form the same sums in the same order: the same bits (tests/test_gpu_align_labels.py).
// alpha_t of every frame is kept in the workspace ((T + 1) * S doubles) by the forward pass when posteriors are wanted; without them the
// forward pass runs alone on its two alternating vectors.  Under option align_checkpoint (the *_ckpt_kernel forms; fb_utterance, CKPT) the
// forward pass keeps alpha of every C-th frame only and the backward pass recomputes a segment's alphas before it walks the segment.
//  * LDS: the two state vectors are 2 * Smax doubles of dynamic LDS, else they lie in the workspace;
//  * ALDS (LDS, posteriors): a third vector holds alpha_t: loaded from the workspace into kAlignFbAlphaRegs registers before step 1, stored
//    to LDS behind it, so the loads' latency hides behind step 1; else step 2 gathers alpha_t from the workspace;
//  * YLDS: two output rows behind the vectors, staged one frame ahead through registers as align_kernels.h does (backward: one frame behind).
#pragma once
#include "align_kernels.h"

namespace tdnnf {
namespace {

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

// the running log-sum of a row's candidates; keep (may be null): a second copy of the results
struct AlignLseAcc {
  double *out, *keep;
  double m, s;
  __device__ __forceinline__ void reset() {
    m = -INFINITY;
    s = 0.0;
  }
  // (no branch around the exp of a batch's padding, which enters as -inf: skipping it where a whole wave is past its rows' ends measured
  // 1 % faster on the 4 000-state graph and 11 % slower on transcript graphs, whose slices mix lengths: docs/experiments.md r6-p)
  __device__ __forceinline__ void take(double v, int, bool valid) { fb_lse_add(m, s, valid ? v : -INFINITY); }
  __device__ __forceinline__ void wave() { fb_lse_wave(m, s); }
  __device__ __forceinline__ void store(int row) {
    const double r = fb_lse_value(m, s);
    out[row] = r;
    if (keep) keep[row] = r;
  }
};

// The forward pass of one utterance on its workgroup: alpha_0 = init into cur, T steps over the arcs by destination on the alternating
// vectors cur / nxt (on return cur is alpha_T), then the total over the final states.  KEEP: alpha_t of every frame goes to alpha,
// (T + 1) * S doubles.  (A compile-time choice: with a test of the pointer in every frame, and the step indexing its slots from the table's
// start, the numerator's recursion on transcripts took 0.399 ms where it takes 0.384: docs/experiments.md r6-r.)
// Returns the log-sum, the same in every thread.
// KEEP = kFbKeepEvery (CKPT below): alpha_t only of the frames t = kC < T, k = 0, 1 .. -- the checkpoints, vector k of alpha.
constexpr int kFbKeepEvery = 2;
template <int NT, bool YLDS, int KEEP>
__device__ __forceinline__ double fb_forward(const AlignDev &g, const AlignGraphDev &gr, int T, AlignRowStage<NT, YLDS> &rows, double scale, double *&cur,
                                             double *&nxt, double *alpha, int C = 0) {
  __shared__ double red_m[NT / 64], red_s[NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, S = gr.num_states, s0 = gr.state0;
  for (int s = tid; s < S; s += NT) {
    const double v = (double)g.init[s0 + s];
    cur[s] = v;
    if (KEEP) alpha[s] = v;
  }
  rows.load(0);
  rows.store(0);
  rows.load(1);
  __syncthreads();
  for (int t = 0; t < T; t++) {
    // row t + 1 (loaded a frame ago) into the buffer whose last readers -- frame t - 1 -- are behind the previous barrier; row t + 2 on its way
    rows.store(t + 1);
    rows.load(t + 2);
    // (KEEP = kFbKeepEvery, t + 1 < T: a checkpoint at T would be vector ceil(T / C), the first of the segment buffer)
    align_step<NT>(g.by_dst, gr.by_dst, cur, rows.row(t), scale,
                   AlignLseAcc{nxt, KEEP == kFbKeepEvery ? (t + 1 < T && (t + 1) % C == 0 ? alpha + (size_t)((t + 1) / C) * S : nullptr)
                                    : KEEP             ? alpha + (size_t)(t + 1) * S
                                                       : nullptr});
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
  return fb_lse_value(m, sum);
}

// One frame's posteriors from one graph's rows of the arcs by pdf: emit(p, column of p, sum over the arcs of pdf p of exp(alpha[src] + term +
// beta[dst] - logprob)), by the element's one owner -- a lane per light pdf, lane 0 of the wave that walks a heavy one -- with the arcs in
// the caller's order.  Only the pdfs that an arc names have a row; a row's column (align_tables.h) comes with its slot or descriptor.
template <int NT, class Emit>
__device__ __forceinline__ void fb_post_step(const AlignTable &tb, const AlignRange &r, const double *alpha, const double *beta, const float *yrow,
                                             double scale, double logprob, Emit emit) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int4 *slots = tb.slots + r.slot0, *heavy = tb.heavy + r.heavy0;
  for (int slot = tid; slot < r.num_slots; slot += NT) {
    const int4 row = slots[slot];
    if (row.x < 0) continue;
    const double ay = scale * (double)yrow[row.x];
    double sum = 0.0;
    for (int j = 0; j < row.y; j += kAlignBatch) {
      int4 arc[kAlignBatch];
#pragma unroll
      for (int k = 0; k < kAlignBatch; k++) arc[k] = tb.arcs[row.z + 64 * min(j + k, row.y - 1)];
#pragma unroll
      for (int k = 0; k < kAlignBatch; k++) {
        const double v = (alpha[arc[k].x] + ((double)__int_as_float(arc[k].z) + ay)) + beta[arc[k].y];
        if (j + k < row.y && v > -INFINITY) sum += exp(v - logprob);
      }
    }
    emit(row.x, row.w, sum);
  }
  for (int h = wave; h < r.num_heavy; h += NT / 64) {
    const int4 row = heavy[h];
    const double ay = scale * (double)yrow[row.x];
    double sum = 0.0;
    for (int a = row.y + lane; a < row.z; a += 64) {
      const int4 arc = tb.arcs[a];
      const double v = (alpha[arc.x] + ((double)__int_as_float(arc.z) + ay)) + beta[arc.y];
      if (v > -INFINITY) sum += exp(v - logprob);
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) emit(row.x, row.w, sum);
  }
}

// The same walk over one graph's rows of the arcs by label: emit(row, column of the label, sum over the arcs with that label of
// exp(alpha[src] + term + beta[dst] - logprob)).  A label's arcs name different pdfs, so the arc carries its pdf (arc.w) and y[t, pdf] is
// read per arc -- from the staged row in LDS or, where rows are not staged, from global memory behind the arc's own load, as align_step
// gathers -- where fb_post_step reads it once per row.  The sum is formed in fb_post_step's association.
template <int NT, class Emit>
__device__ __forceinline__ void fb_label_step(const AlignTable &tb, const AlignRange &r, const double *alpha, const double *beta, const float *yrow,
                                              double scale, double logprob, Emit emit) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int4 *slots = tb.slots + r.slot0, *heavy = tb.heavy + r.heavy0;
  for (int slot = tid; slot < r.num_slots; slot += NT) {
    const int4 row = slots[slot];
    if (row.x < 0) continue;
    double sum = 0.0;
    for (int j = 0; j < row.y; j += kAlignBatch) {
      int4 arc[kAlignBatch];
      float yv[kAlignBatch];
#pragma unroll
      for (int k = 0; k < kAlignBatch; k++) arc[k] = tb.arcs[row.z + 64 * min(j + k, row.y - 1)];
#pragma unroll
      for (int k = 0; k < kAlignBatch; k++) yv[k] = yrow[arc[k].w];
#pragma unroll
      for (int k = 0; k < kAlignBatch; k++) {
        const double v = (alpha[arc[k].x] + ((double)__int_as_float(arc[k].z) + scale * (double)yv[k])) + beta[arc[k].y];
        if (j + k < row.y && v > -INFINITY) sum += exp(v - logprob);
      }
    }
    emit(row.x, row.w, sum);
  }
  for (int h = wave; h < r.num_heavy; h += NT / 64) {
    const int4 row = heavy[h];
    double sum = 0.0;
    for (int a = row.y + lane; a < row.z; a += 64) {
      const int4 arc = tb.arcs[a];
      const double v = (alpha[arc.x] + ((double)__int_as_float(arc.z) + scale * (double)yrow[arc.w])) + beta[arc.y];
      if (v > -INFINITY) sum += exp(v - logprob);
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) emit(row.x, row.w, sum);
  }
}

// Step 2 of a frame as fb_utterance takes it: which table is walked, and by which step.
struct FbPdfStep {
  template <int NT, class Emit>
  __device__ __forceinline__ void run(const AlignDev &g, const AlignGraphDev &gr, int, const double *alpha, const double *beta, const float *yrow,
                                      double scale, double logprob, Emit emit) const {
    fb_post_step<NT>(g.by_pdf, gr.by_pdf, alpha, beta, yrow, scale, logprob, emit);
  }
};
struct FbLabelStep {
  AlignTable by_label;       // tdnnf_align_graphs::by_label
  const AlignRange *ranges;  // [graphs]: the graphs' shares of it (tdnnf_align_graphs::label_range_dev)
  template <int NT, class Emit>
  __device__ __forceinline__ void run(const AlignDev &, const AlignGraphDev &, int graph, const double *alpha, const double *beta, const float *yrow,
                                      double scale, double logprob, Emit emit) const {
    fb_label_step<NT>(by_label, ranges[graph], alpha, beta, yrow, scale, logprob, emit);
  }
};

// Where an utterance's posteriors go.  frame(t) before the owners of frame t emit(pdf, column, value), with a workgroup barrier in between;
// fail(T): the utterance has no finite logprob, all it owns becomes 0.
// Dense: row utt_row_begin + t * row_stride of a matrix of P columns, element [t, pdf]; the pdfs no arc names have no owner, so frame(t)
// zeroes the row first.
template <int NT>
struct FbDenseOut {
  MatView post;
  int row_begin, row_stride, P;
  float *prow;
  __device__ __forceinline__ float *row(int t) const { return post.data + (size_t)(row_begin + (long long)t * row_stride) * post.stride; }
  __device__ __forceinline__ void fail(int T) {
    for (int t = 0; t < T; t++) {
      prow = row(t);
      for (int c = threadIdx.x; c < P; c += NT) prow[c] = 0.f;
    }
  }
  __device__ __forceinline__ void frame(int t) {
    prow = row(t);
    for (int c = threadIdx.x; c < P; c += NT) prow[c] = 0.f;
  }
  __device__ __forceinline__ void emit(int pdf, int, float v) { prow[pdf] = v; }
};
// Compact: the utterance's block of T rows of D floats, D the distinct pdfs of its graph, element [t, column]: every column has an owner
// in every frame, so nothing is zeroed.
template <int NT>
struct FbCompactOut {
  float *block;
  int D;
  float *prow;
  __device__ __forceinline__ void fail(int T) {
    for (size_t i = threadIdx.x; i < (size_t)T * D; i += NT) block[i] = 0.f;
  }
  __device__ __forceinline__ void frame(int t) { prow = block + (size_t)t * D; }
  __device__ __forceinline__ void emit(int, int column, float v) { prow[column] = v; }
};

// The backward pass of fb_utterance over an alpha region with checkpoints (CKPT there; C >= 1 the interval, the layout is AlignCheckpointPlan's,
// align_tables.h): the forward pass has kept alpha_kC, the checkpoint of segment k = [kC, min(kC + C, T)); cur holds beta_T.  The segments
// are taken from the last to the first:
//   a. alpha_kC+1 .. alpha_end-1 again, from the checkpoint into the segment buffer, by the forward pass's own step on the arcs by destination:
//      the same candidates in the same order through the same accumulator, so the bits of the first pass.  beta_end (cur) is live meanwhile.
//      ALDS: nxt and the third vector are free then, and the recursion runs on them (its first step reads the checkpoint from the workspace),
//      the buffer getting the accumulator's second copy; otherwise (LDS without a third vector, the workspace form) each step gathers
//      alpha_t from the buffer in the workspace and writes alpha_t+1 there.
//   b. the frames end - 1 .. kC as fb_utterance takes them -- its frame, word for word, in a function of its own so that the kernels without
//      checkpoints compile to what they were -- with alpha_t from the checkpoint (t = kC) or the buffer.
// The row stage is primed for one direction: it is primed again before a. (forward from kC) and before b. (backward from end - 1), behind the
// barrier that ends the frame before.  A one-frame segment has no a., and its b. goes on with the rows the segment before it staged.
template <int NT, bool YLDS, bool ALDS, class Step, class Out>
__device__ __forceinline__ void fb_backward_ckpt(const AlignDev &g, const AlignGraphDev &gr, int graph, int T, int C, AlignRowStage<NT, YLDS> &rows,
                                                 double scale, double w, double logprob, double *cur, double *nxt, double *alds, double *alpha,
                                                 Step &step, Out &out) {
  const int tid = threadIdx.x, S = gr.num_states;
  const int segments = T > 0 ? (T - 1) / C + 1 : 0;
  double *buffer = alpha + (size_t)segments * S;  // slot j is alpha_begin+1+j of the segment at hand
  for (int k = segments - 1; k >= 0; k--) {
    const int begin = k * C, end = begin + min(C, T - begin);
    const double *checkpoint = alpha + (size_t)k * S;
    if (end - begin > 1) {
      // (the rows' and the vectors' last readers -- frame end, or the total -- are behind a barrier)
      rows.load(begin);
      rows.store(begin);
      rows.load(begin + 1);
      __syncthreads();
      const double *from = checkpoint;
      double *to = nxt, *spare = alds;
      for (int t = begin; t < end - 1; t++) {
        rows.store(t + 1);
        rows.load(t + 2);
        double *slot = buffer + (size_t)(t - begin) * S;
        align_step<NT>(g.by_dst, gr.by_dst, from, rows.row(t), scale, ALDS ? AlignLseAcc{to, slot} : AlignLseAcc{slot, nullptr});
        __syncthreads();
        from = ALDS ? to : slot;
        double *sw = to;
        to = spare;
        spare = sw;
      }
    }
    if (k == segments - 1 || end - begin > 1) {
      rows.load(end - 1);
      rows.store(end - 1);
      rows.load(end - 2);
      __syncthreads();
    }
    for (int t = end - 1; t >= begin; t--) {
      rows.store(t - 1);
      rows.load(t - 2);
      const float *yrow = rows.row(t);
      out.frame(t);
      const double *at = t == begin ? checkpoint : buffer + (size_t)(t - begin - 1) * S;
      double areg[kAlignFbAlphaRegs];
      if (ALDS) {
#pragma unroll
        for (int c = 0; c < kAlignFbAlphaRegs; c++)
          if (tid + c * NT < S) areg[c] = at[tid + c * NT];
      }
      if (t > 0)  // (beta_0 has no reader)
        align_step<NT>(g.by_src, gr.by_src, cur, yrow, scale, AlignLseAcc{nxt, nullptr});
      if (ALDS) {
#pragma unroll
        for (int c = 0; c < kAlignFbAlphaRegs; c++)
          if (tid + c * NT < S) alds[tid + c * NT] = areg[c];
      }
      __syncthreads();  // alpha_t is in place and the row's zeros (dense) are stored
      step.template run<NT>(g, gr, graph, ALDS ? (const double *)alds : at, cur, yrow, scale, logprob,
                            [&](int row, int column, double sum) { out.emit(row, column, (float)(w * sum)); });
      __syncthreads();
      double *sw = cur;
      cur = nxt;
      nxt = sw;
    }
  }
}

// One utterance on its workgroup.  Dynamic LDS: [LDS: 2 * Smax doubles, the state vectors] [ALDS: Smax doubles, alpha_t] [YLDS: 2 * P floats, two output rows].
// POST: alpha_all / out are read and written; otherwise it ends with the total.  step: FbPdfStep or FbLabelStep.
// CKPT (POST; C >= 1 the interval): the forward pass keeps alpha of every C-th frame only and fb_backward_ckpt walks the frames.
template <int NT, bool LDS, bool YLDS, bool ALDS, bool POST, bool CKPT = false, class Step, class MakeOut>
__device__ __forceinline__ void fb_utterance(AlignDev g, const AlignUtt *utts, MatView y, int row_stride, float acoustic_scale, float weight, Step step,
                                             MakeOut make_out, double *alpha_all, double *vecs, double *results, int Smax, int P, int C = 0) {
  static_assert(LDS || !(YLDS || ALDS), "the rows behind the vectors need the LDS form");
  static_assert(POST || !ALDS, "alpha_t is staged for the posteriors only");
  static_assert(POST || !CKPT, "checkpoints are of the alpha kept for the posteriors");
  extern __shared__ double fb_smem[];
  const int tid = threadIdx.x;
  const AlignUtt u = utts[blockIdx.x];
  const AlignGraphDev gr = g.graphs[u.graph];
  const int S = gr.num_states, T = u.frames, s0 = gr.state0;
  double *cur = LDS ? fb_smem : vecs + u.vec_begin, *nxt = cur + S;
  double *alds = fb_smem + 2 * (size_t)Smax;  // ALDS: alpha_t
  double *alpha = POST ? alpha_all + u.frame_begin : nullptr;
  const double scale = (double)acoustic_scale;
  AlignRowStage<NT, YLDS> rows(y.data + (size_t)u.row_begin * y.stride, (size_t)row_stride * y.stride, P, T,
                               reinterpret_cast<float *>(fb_smem + (ALDS ? 3 : 2) * (size_t)Smax));
  const double logprob = fb_forward<NT, YLDS, CKPT ? kFbKeepEvery : POST>(g, gr, T, rows, scale, cur, nxt, alpha, C);
  const bool ok = logprob > -INFINITY && logprob < INFINITY;
  if (tid == 0) {
    results[2 * (size_t)blockIdx.x] = logprob;
    results[2 * (size_t)blockIdx.x + 1] = ok ? 1.0 : 0.0;
  }
  if (!POST) return;
  auto out = make_out(u);
  if (!ok) {
    out.fail(T);
    return;
  }
  const double w = (double)weight;
  // (alpha_T's last readers are behind the barrier above)
  for (int s = tid; s < S; s += NT) cur[s] = (double)g.final[s0 + s];
  if constexpr (CKPT) {
    fb_backward_ckpt<NT, YLDS, ALDS>(g, gr, u.graph, T, C, rows, scale, w, logprob, cur, nxt, alds, alpha, step, out);
    return;
  }
  rows.load(T - 1);
  rows.store(T - 1);
  rows.load(T - 2);
  __syncthreads();
  for (int t = T - 1; t >= 0; t--) {
    // row t - 1 into the buffer whose last readers -- frame t + 1 -- are behind the previous barrier; row t - 2 on its way
    rows.store(t - 1);
    rows.load(t - 2);
    const float *yrow = rows.row(t);
    out.frame(t);
    const double *at = alpha + (size_t)t * S;
    double areg[kAlignFbAlphaRegs];
    if (ALDS) {
#pragma unroll
      for (int c = 0; c < kAlignFbAlphaRegs; c++)
        if (tid + c * NT < S) areg[c] = at[tid + c * NT];
    }
    if (t > 0)  // (beta_0 has no reader)
      align_step<NT>(g.by_src, gr.by_src, cur, yrow, scale, AlignLseAcc{nxt, nullptr});
    if (ALDS) {
#pragma unroll
      for (int c = 0; c < kAlignFbAlphaRegs; c++)
        if (tid + c * NT < S) alds[tid + c * NT] = areg[c];
    }
    __syncthreads();  // alpha_t is in place and the row's zeros (dense) are stored
    step.template run<NT>(g, gr, u.graph, ALDS ? (const double *)alds : at, cur, yrow, scale, logprob,
                          [&](int row, int column, double sum) { out.emit(row, column, (float)(w * sum)); });
    __syncthreads();
    double *sw = cur;
    cur = nxt;
    nxt = sw;
  }
}

// grid = utterances.  The dense form: post is addressed like y.
template <int NT, bool LDS, bool YLDS, bool ALDS, bool POST>
__global__ __launch_bounds__(NT) void align_fb_kernel(AlignDev g, const AlignUtt *utts, MatView y, int row_stride, float acoustic_scale, float weight,
                                                      MatView post, double *alpha_all, double *vecs, double *results, int Smax, int P) {
  fb_utterance<NT, LDS, YLDS, ALDS, POST>(
      g, utts, y, row_stride, acoustic_scale, weight, FbPdfStep{},
      [&](const AlignUtt &u) { return FbDenseOut<NT>{post, u.row_begin, row_stride, P, nullptr}; }, alpha_all, vecs, results, Smax, P);
}

// grid = utterances.  The compact form (always with posteriors): utterance u's block starts at compact + u.out_begin and has
// graph_cols[u.graph] floats a frame.
template <int NT, bool LDS, bool YLDS, bool ALDS>
__global__ __launch_bounds__(NT) void align_fb_compact_kernel(AlignDev g, const AlignUtt *utts, MatView y, int row_stride, float acoustic_scale,
                                                              float weight, float *compact, const int *graph_cols, double *alpha_all, double *vecs,
                                                              double *results, int Smax, int P) {
  fb_utterance<NT, LDS, YLDS, ALDS, true>(
      g, utts, y, row_stride, acoustic_scale, weight, FbPdfStep{},
      [&](const AlignUtt &u) { return FbCompactOut<NT>{compact + u.out_begin, graph_cols[u.graph], nullptr}; }, alpha_all, vecs, results, Smax, P);
}

// grid = utterances.  The label form: the compact form with step 2 on the arcs by label; graph_cols[u.graph] is the number of distinct
// labels of the utterance's graph, label_ranges[u.graph] its share of by_label.
template <int NT, bool LDS, bool YLDS, bool ALDS>
__global__ __launch_bounds__(NT) void align_fb_label_kernel(AlignDev g, AlignTable by_label, const AlignRange *label_ranges, const AlignUtt *utts, MatView y,
                                                            int row_stride, float acoustic_scale, float weight, float *compact, const int *graph_cols,
                                                            double *alpha_all, double *vecs, double *results, int Smax, int P) {
  fb_utterance<NT, LDS, YLDS, ALDS, true>(
      g, utts, y, row_stride, acoustic_scale, weight, FbLabelStep{by_label, label_ranges},
      [&](const AlignUtt &u) { return FbCompactOut<NT>{compact + u.out_begin, graph_cols[u.graph], nullptr}; }, alpha_all, vecs, results, Smax, P);
}

// The three kernels above with alpha checkpoints (fb_utterance, CKPT): the same arguments and C >= 1, the call's interval, behind them.
// Kernels of their own, so that a call without checkpoints launches what it launched before there were any.
template <int NT, bool LDS, bool YLDS, bool ALDS>
__global__ __launch_bounds__(NT) void align_fb_ckpt_kernel(AlignDev g, const AlignUtt *utts, MatView y, int row_stride, float acoustic_scale, float weight,
                                                           MatView post, double *alpha_all, double *vecs, double *results, int Smax, int P, int C) {
  fb_utterance<NT, LDS, YLDS, ALDS, true, true>(
      g, utts, y, row_stride, acoustic_scale, weight, FbPdfStep{},
      [&](const AlignUtt &u) { return FbDenseOut<NT>{post, u.row_begin, row_stride, P, nullptr}; }, alpha_all, vecs, results, Smax, P, C);
}

template <int NT, bool LDS, bool YLDS, bool ALDS>
__global__ __launch_bounds__(NT) void align_fb_compact_ckpt_kernel(AlignDev g, const AlignUtt *utts, MatView y, int row_stride, float acoustic_scale,
                                                                   float weight, float *compact, const int *graph_cols, double *alpha_all, double *vecs,
                                                                   double *results, int Smax, int P, int C) {
  fb_utterance<NT, LDS, YLDS, ALDS, true, true>(
      g, utts, y, row_stride, acoustic_scale, weight, FbPdfStep{},
      [&](const AlignUtt &u) { return FbCompactOut<NT>{compact + u.out_begin, graph_cols[u.graph], nullptr}; }, alpha_all, vecs, results, Smax, P, C);
}

template <int NT, bool LDS, bool YLDS, bool ALDS>
__global__ __launch_bounds__(NT) void align_fb_label_ckpt_kernel(AlignDev g, AlignTable by_label, const AlignRange *label_ranges, const AlignUtt *utts,
                                                                 MatView y, int row_stride, float acoustic_scale, float weight, float *compact,
                                                                 const int *graph_cols, double *alpha_all, double *vecs, double *results, int Smax, int P,
                                                                 int C) {
  fb_utterance<NT, LDS, YLDS, ALDS, true, true>(
      g, utts, y, row_stride, acoustic_scale, weight, FbLabelStep{by_label, label_ranges},
      [&](const AlignUtt &u) { return FbCompactOut<NT>{compact + u.out_begin, graph_cols[u.graph], nullptr}; }, alpha_all, vecs, results, Smax, P, C);
}

}  // namespace
}  // namespace tdnnf
