// align_kernels.h -- what every recursion over the tables of a tdnnf_align_graphs shares on the device (AlignRowStage, align_step), and the
// best path (Viterbi) through cyclic, epsilon-free acceptors with pdf-ids on their arcs: forced alignment on transcript graphs, free
// decoding on the denominator graph.  align.hip launches align_best_path_kernel; align_fb_kernels.h and num_e2e_kernels.h build the
// log-sum recursions on the shared parts.  The tables' layout: align_tables.h.
//
// Arithmetic (held bit for bit by tests/test_gpu_align.py against tests/viterbi_ref64.py):
//     term(arc, t) = (double)arc_logprob + (double)acoustic_scale * (double)y[t, arc_pdf]      (the product of two floats is exact in double,
//                                                                                               so a fused multiply-add rounds the same once)
//     alpha_0[s]   = (double)initial_logprob[s]
//     alpha_t+1[d] = max over arcs into d of  alpha_t[src] + term(arc, t)
//     score        = max over s of  alpha_T[s] + (double)final_logprob[s]
//   No clamp on y (the numerator applies none).  -inf is "not reachable" / "not final"; an arc is a candidate only if its sum compares
//   GREATER than the best so far, which starts at -inf: a sum of -inf or NaN is never chosen and a NaN never enters a state vector.
//   Ties: the arc that comes first in the caller's arc list wins (the arcs of a destination keep the caller's order, a thread walks them
//   in order with a strict >, and partial results are merged by (greater value, then lower position)); among equal final states the
//   lowest state wins.  No accepting path of the utterance's length: ok = 0, score = -inf, every pdf-id (and state) -1.  A score of
//   +inf: ok = 0 as well, the score is reported as it is.
//
// One workgroup per utterance walks the frames in order; workgroup barriers are the only synchronisation (no agent-scope exchange, no
// polling, no co-residency requirement) and every loop is bounded by the frame count, the state count or an arc range.
//  * state scores: two vectors of S doubles, alternating -- in LDS (LDS form) or in the workspace (global form).
//  * arcs (align_step): a lane per light row, slice by slice; kAlignBatch arcs are loaded before their output elements, and those before
//    the first comparison: one round trip to the L2 per batch instead of two per arc.  A wave per heavy row behind the light ones: the
//    lanes stride the row's contiguous arcs, and a butterfly merges the 64 partial results.
//  * gather (AlignRowStage): where two output rows of P floats fit the LDS behind the vectors and a thread can carry its share of a row in
//    kAlignRowRegs registers, the row of frame t + 1 is loaded coalesced while frame t is worked on and y[t, pdf] is an LDS read (as
//    num_wide_kernels.h gathers one frame ahead; 24 -> 10 us per frame on the 4 000-state graph); otherwise y[t, pdf] is a global load
//    behind the arc's.
//  * back-pointers: bp[t * S + d] = position (in the arc table) of the arc chosen for state d at frame t + 1, or -1.
//  * trace-back: one thread walks the back-pointers from the best final state and leaves the chosen arc of frame t in bp[t * S];
//    behind a barrier the workgroup writes pdf-ids (and states) coalesced.
//  * labels (align_path_labels_kernel, behind the best path on its stream): bp[t * S] still holds the chosen arc of frame t, whose 4th
//    int is the caller's arc index; a thread per (utterance, frame) writes that index and the caller's label of the arc.
//  * option align_path_checkpoint (align_best_path_ckpt_kernel, align_path_labels_ckpt_kernel, at the end): the state scores of every C-th
//    frame and the back-pointers of C frames at a time; the trace-back recomputes each earlier segment's back-pointers from its checkpoint.
#pragma once
#include "align_graphs.h"

namespace tdnnf {
namespace {

constexpr int kAlignBatch = 4;  // arcs of a light row loaded together

// The output rows of one utterance: row t lies t * step elements behind row0.  YLDS (P <= kAlignRowRegs * NT): ylds holds two rows of P
// floats, used alternately -- a frame's row is loaded coalesced into registers one frame before it is stored to the LDS and two before it
// is read, so an arc's y[t, pdf] is an LDS read instead of a global load that has to wait for the arc's own load.  Frames outside [0, T)
// are skipped: the walk runs forward (load t + 2, store t + 1) or backward (load t - 2, store t - 1) without minding the ends.
template <int NT, bool YLDS>
struct AlignRowStage {
  const float *row0;
  size_t step;
  int P, T;
  float *ylds;
  float yreg[kAlignRowRegs];
  __device__ __forceinline__ AlignRowStage(const float *row0, size_t step, int P, int T, float *ylds) : row0(row0), step(step), P(P), T(T), ylds(ylds) {}
  __device__ __forceinline__ void load(int t) {  // (only [0, P) of a row: what the graphs' arcs can name)
    if (!YLDS || t < 0 || t >= T) return;
    const float *r = row0 + (size_t)t * step;
    const int tid = threadIdx.x;
#pragma unroll
    for (int c = 0; c < kAlignRowRegs; c++)
      if (tid + c * NT < P) yreg[c] = r[tid + c * NT];
  }
  __device__ __forceinline__ void store(int t) {
    if (!YLDS || t < 0 || t >= T) return;
    const int tid = threadIdx.x;
#pragma unroll
    for (int c = 0; c < kAlignRowRegs; c++)
      if (tid + c * NT < P) ylds[(size_t)(t & 1) * P + tid + c * NT] = yreg[c];
  }
  __device__ __forceinline__ const float *row(int t) const { return YLDS ? ylds + (size_t)(t & 1) * P : row0 + (size_t)t * step; }
};

// One frame of a recursion on one graph's rows of one table: every row's candidates from[arc.x] + term(arc), in the caller's order, go to
// the accumulator.  Forward: the arcs by destination, arc.x the source; backward: the arcs by source, arc.x the destination.
// Acc: reset() before a row; take(candidate, its position in the arc table, whether it is an arc and not a batch's padding); wave() merges
// the 64 lanes' partial results of a heavy row; store(row) writes the row's result.
template <int NT, class Acc>
__device__ __forceinline__ void align_step(const AlignTable &tb, const AlignRange &r, const double *from, const float *yrow, double scale, Acc acc) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int4 *slots = tb.slots + r.slot0, *heavy = tb.heavy + r.heavy0;  // (offset once: the compiler lifts these out of the frame loop)
  for (int slot = tid; slot < r.num_slots; slot += NT) {  // light rows: a lane per row, slice by slice
    const int4 row = slots[slot];
    if (row.x < 0) continue;
    acc.reset();
    for (int j = 0; j < row.y; j += kAlignBatch) {
      int4 arc[kAlignBatch];
      float yv[kAlignBatch];
#pragma unroll
      for (int k = 0; k < kAlignBatch; k++) arc[k] = tb.arcs[row.z + 64 * min(j + k, row.y - 1)];
#pragma unroll
      for (int k = 0; k < kAlignBatch; k++) yv[k] = yrow[arc[k].y];
#pragma unroll
      for (int k = 0; k < kAlignBatch; k++)
        acc.take(from[arc[k].x] + ((double)__int_as_float(arc[k].z) + scale * (double)yv[k]), row.z + 64 * (j + k), j + k < row.y);
    }
    acc.store(row.x);
  }
  for (int h = wave; h < r.num_heavy; h += NT / 64) {  // heavy rows: a wave per row
    const int4 row = heavy[h];
    acc.reset();
    for (int a = row.y + lane; a < row.z; a += 64) {
      const int4 arc = tb.arcs[a];
      acc.take(from[arc.x] + ((double)__int_as_float(arc.z) + scale * (double)yrow[arc.y]), a, true);
    }
    acc.wave();
    if (lane == 0) acc.store(row.x);
  }
}

// (value, position): the greater value, among equal values the lower position
__device__ __forceinline__ void align_merge(double &v, int &p, double ov, int op) {
  if (ov > v || (ov == v && op >= 0 && (p < 0 || op < p))) {
    v = ov;
    p = op;
  }
}
__device__ __forceinline__ void align_wave_best(double &v, int &p) {
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o, 64);
    const int op = __shfl_xor(p, o, 64);
    align_merge(v, p, ov, op);
  }
}

// the best candidate and its position under a strict >: the first of equals wins, padding is not taken
struct AlignBestAcc {
  double *out;
  int *bp;
  double best;
  int bi;
  __device__ __forceinline__ void reset() {
    best = -INFINITY;
    bi = -1;
  }
  __device__ __forceinline__ void take(double v, int pos, bool valid) {
    if (valid && v > best) {
      best = v;
      bi = pos;
    }
  }
  __device__ __forceinline__ void wave() { align_wave_best(best, bi); }
  __device__ __forceinline__ void store(int row) {
    out[row] = best;
    bp[row] = bi;
  }
};

// grid = utterances.  LDS: the two state vectors are 2 * Smax doubles of dynamic LDS; otherwise vecs + u.vec_begin.
// YLDS (LDS only): behind the vectors the LDS holds the two output rows of AlignRowStage.
template <int NT, bool LDS, bool YLDS>
__global__ __launch_bounds__(NT) void align_best_path_kernel(AlignDev g, const AlignUtt *utts, MatView y, int row_stride, float acoustic_scale,
                                                             int *bp_all, double *vecs, int *pdf_out, int *state_out, double *results, int Smax, int P) {
  extern __shared__ double align_smem[];
  __shared__ double red_v[NT / 64];
  __shared__ int red_p[NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const AlignUtt u = utts[blockIdx.x];
  const AlignGraphDev gr = g.graphs[u.graph];
  const int S = gr.num_states, T = u.frames, s0 = gr.state0;
  double *cur = LDS ? align_smem : vecs + u.vec_begin, *nxt = cur + S;
  int *bp = bp_all + u.frame_begin;
  const double scale = (double)acoustic_scale;
  AlignRowStage<NT, YLDS> rows(y.data + (size_t)u.row_begin * y.stride, (size_t)row_stride * y.stride, P, T,
                               reinterpret_cast<float *>(align_smem + 2 * (size_t)Smax));
  for (int s = tid; s < S; s += NT) cur[s] = (double)g.init[s0 + s];
  rows.load(0);
  rows.store(0);
  rows.load(1);
  __syncthreads();
  for (int t = 0; t < T; t++) {
    // row t + 1 (loaded a frame ago) into the buffer whose last readers -- frame t - 1 -- are behind the previous barrier; row t + 2 on its way
    rows.store(t + 1);
    rows.load(t + 2);
    align_step<NT>(g.by_dst, gr.by_dst, cur, rows.row(t), scale, AlignBestAcc{nxt, bp + (size_t)t * S});
    __syncthreads();
    double *sw = cur;
    cur = nxt;
    nxt = sw;
  }
  // the best final state: the lowest state among equal scores
  double best = -INFINITY;
  int bs = -1;
  for (int s = tid; s < S; s += NT) {
    const double v = cur[s] + (double)g.final[s0 + s];
    if (v > best) {
      best = v;
      bs = s;
    }
  }
  align_wave_best(best, bs);
  if (lane == 0) {
    red_v[wave] = best;
    red_p[wave] = bs;
  }
  __syncthreads();
  best = red_v[0];  // (every thread merges the waves' results alike: what follows branches on them workgroup-wide)
  bs = red_p[0];
  for (int w = 1; w < NT / 64; w++) align_merge(best, bs, red_v[w], red_p[w]);
  const bool ok = bs >= 0 && best < INFINITY;
  if (tid == 0) {
    results[2 * (size_t)blockIdx.x] = best;
    results[2 * (size_t)blockIdx.x + 1] = ok ? 1.0 : 0.0;
  }
  int *pdfs = pdf_out + u.out_begin, *states = state_out ? state_out + u.out_begin + blockIdx.x : nullptr;
  if (!ok) {
    for (int t = tid; t < T; t += NT) pdfs[t] = -1;
    if (states)
      for (int t = tid; t <= T; t += NT) states[t] = -1;
    return;
  }
  const int4 *arcs = g.by_dst.arcs;
  if (tid == 0) {  // (a reachable state at frame t + 1 has a chosen arc, whose source was reachable at frame t: no -1 on this walk; guarded all the same)
    int st = bs;
    for (int t = T - 1; t >= 0; t--) {
      const int a = bp[(size_t)t * S + st];
      if (a >= 0) st = arcs[a].x;
      bp[(size_t)t * S] = a;
    }
  }
  __syncthreads();
  for (int t = tid; t < T; t += NT) {
    const int a = bp[(size_t)t * S];
    const int4 arc = a >= 0 ? arcs[a] : make_int4(-1, -1, 0, -1);
    pdfs[t] = arc.y;
    if (states) states[t] = arc.x;
  }
  if (states && tid == 0) states[T] = bs;
}

// grid = (frames of the longest utterance / NT, utterances), behind align_best_path_kernel on the same stream: what the trace-back left in
// bp_all (the chosen arc of frame t at bp[t * S]) becomes arc_out[t], the caller's arc index (global over the graphs), and label_out[t],
// arc_label of that arc; -1 both for an utterance the best path gave ok = 0.  arc_out may be null.  Consecutive threads write consecutive
// elements; every element of the utterance's share of both outputs is written.
template <int NT>
__global__ __launch_bounds__(NT) void align_path_labels_kernel(AlignDev g, const AlignUtt *utts, const int *bp_all, const double *results,
                                                               const int *arc_label, int *label_out, int *arc_out) {
  const AlignUtt u = utts[blockIdx.y];
  const int t = blockIdx.x * NT + threadIdx.x;
  if (t >= u.frames) return;
  int arc = -1, label = -1;
  if (results[2 * (size_t)blockIdx.y + 1] != 0.0) {
    const int a = bp_all[u.frame_begin + (long long)t * g.graphs[u.graph].num_states];
    if (a >= 0) {  // (guarded as the trace-back guards it)
      arc = g.by_dst.arcs[a].w;
      label = arc_label[arc];
    }
  }
  label_out[u.out_begin + t] = label;
  if (arc_out) arc_out[u.out_begin + t] = arc;
}

// ---- option align_path_checkpoint: back-pointers of one segment of C frames at a time (the layout: align_tables.h AlignPathCheckpointPlan)
// An utterance's region starts at ints + u.frame_begin (an even count of ints: 8-byte aligned): K = ceil(T / C) checkpoints of S doubles, the
// segment buffer of min(C, T) * S ints and the path of T ints, buffer and path padded to an even count.
struct AlignPathRegions {
  double *ck;  // alpha_kC at ck + k * S
  int *buf;    // the back-pointers of frame kC + j of the segment last swept at buf + j * S
  int *path;   // the chosen arc of frame t
};
__device__ __forceinline__ AlignPathRegions align_path_regions(int *ints, const AlignUtt &u, int S, int C) {
  const size_t K = u.frames > 0 ? (size_t)(u.frames - 1) / C + 1 : 0, B = (size_t)min(C, u.frames);
  AlignPathRegions r;
  int *base = ints + u.frame_begin;
  r.ck = reinterpret_cast<double *>(base);
  r.buf = base + 2 * K * (size_t)S;
  r.path = r.buf + (B * (size_t)S + 1) / 2 * 2;
  return r;
}

// align_best_path_kernel under the option, C >= 1 the interval (at most the call's longest utterance): the same launch, the same arguments
// and C; bp_all is the per-frame region of the workspace.  The forward pass is the recursion above; at every segment start kC it also
// stores alpha_kC (the vector it is about to read) to the utterance's checkpoints, coalesced, and its back-pointers go to the segment buffer,
// each segment over the one before: at the end the buffer holds the last segment's.  The trace-back walks that segment, then for k = K - 2
// .. 0 the workgroup reloads alpha_kC, reruns the segment's C frames by the forward pass's own step -- max and + in double on the same
// operands in the same order: the same back-pointers -- and thread 0 walks on from the state it had reached.  The rows of AlignRowStage are
// primed again at every segment start.  The chosen arcs go to the path region, which the coalesced write of the outputs (and
// align_path_labels_ckpt_kernel) reads.  T <= C is one segment: nothing is recomputed.  An utterance with ok = 0 writes its -1s and is done.
// The frame body is written here a second time (and a third, for the rerun) so that align_best_path_kernel's device code is what it was.
template <int NT, bool LDS, bool YLDS>
__global__ __launch_bounds__(NT) void align_best_path_ckpt_kernel(AlignDev g, const AlignUtt *utts, MatView y, int row_stride, float acoustic_scale,
                                                                  int *bp_all, double *vecs, int *pdf_out, int *state_out, double *results, int Smax, int P,
                                                                  int C) {
  extern __shared__ double align_smem[];
  __shared__ double red_v[NT / 64];
  __shared__ int red_p[NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const AlignUtt u = utts[blockIdx.x];
  const AlignGraphDev gr = g.graphs[u.graph];
  const int S = gr.num_states, T = u.frames, s0 = gr.state0;
  double *cur = LDS ? align_smem : vecs + u.vec_begin, *nxt = cur + S;
  const AlignPathRegions rg = align_path_regions(bp_all, u, S, C);
  const double scale = (double)acoustic_scale;
  AlignRowStage<NT, YLDS> rows(y.data + (size_t)u.row_begin * y.stride, (size_t)row_stride * y.stride, P, T,
                               reinterpret_cast<float *>(align_smem + 2 * (size_t)Smax));
  for (int s = tid; s < S; s += NT) cur[s] = (double)g.init[s0 + s];
  rows.load(0);
  rows.store(0);
  rows.load(1);
  __syncthreads();
  int last = 0;  // the first frame of the segment whose back-pointers the buffer holds
  for (int t = 0, j = 0; t < T; t++, j++) {
    if (j == C) j = 0;
    if (j == 0) {  // a segment starts: alpha_t (complete behind the last barrier, read-only in this frame) is its checkpoint
      last = t;
      double *ck = rg.ck + (size_t)(t / C) * S;
      for (int s = tid; s < S; s += NT) ck[s] = cur[s];
    }
    rows.store(t + 1);
    rows.load(t + 2);
    align_step<NT>(g.by_dst, gr.by_dst, cur, rows.row(t), scale, AlignBestAcc{nxt, rg.buf + (size_t)j * S});
    __syncthreads();
    double *sw = cur;
    cur = nxt;
    nxt = sw;
  }
  // the best final state: the lowest state among equal scores
  double best = -INFINITY;
  int bs = -1;
  for (int s = tid; s < S; s += NT) {
    const double v = cur[s] + (double)g.final[s0 + s];
    if (v > best) {
      best = v;
      bs = s;
    }
  }
  align_wave_best(best, bs);
  if (lane == 0) {
    red_v[wave] = best;
    red_p[wave] = bs;
  }
  __syncthreads();
  best = red_v[0];  // (every thread merges the waves' results alike: what follows branches on them workgroup-wide)
  bs = red_p[0];
  for (int w = 1; w < NT / 64; w++) align_merge(best, bs, red_v[w], red_p[w]);
  const bool ok = bs >= 0 && best < INFINITY;
  if (tid == 0) {
    results[2 * (size_t)blockIdx.x] = best;
    results[2 * (size_t)blockIdx.x + 1] = ok ? 1.0 : 0.0;
  }
  int *pdfs = pdf_out + u.out_begin, *states = state_out ? state_out + u.out_begin + blockIdx.x : nullptr;
  if (!ok) {
    for (int t = tid; t < T; t += NT) pdfs[t] = -1;
    if (states)
      for (int t = tid; t <= T; t += NT) states[t] = -1;
    return;
  }
  const int4 *arcs = g.by_dst.arcs;
  int st = bs;  // (thread 0's: the state the trace-back has reached)
  for (int b = last, e = T; e > 0; e = b, b -= C) {  // the segments [b, e) from the last to the first; every b is a multiple of C
    if (e < T) {
      // (behind this barrier thread 0 has walked the buffer, and every reader of the state vectors and of the staged rows is done)
      __syncthreads();
      const double *ck = rg.ck + (size_t)(b / C) * S;
      for (int s = tid; s < S; s += NT) cur[s] = ck[s];
      rows.load(b);
      rows.store(b);
      rows.load(b + 1);
      __syncthreads();
      for (int t = b; t < e; t++) {
        rows.store(t + 1);
        rows.load(t + 2);
        align_step<NT>(g.by_dst, gr.by_dst, cur, rows.row(t), scale, AlignBestAcc{nxt, rg.buf + (size_t)(t - b) * S});
        __syncthreads();
        double *sw = cur;
        cur = nxt;
        nxt = sw;
      }
    }
    if (tid == 0) {  // (as in align_best_path_kernel: no -1 on this walk; guarded all the same)
      for (int t = e - 1; t >= b; t--) {
        const int a = rg.buf[(size_t)(t - b) * S + st];
        if (a >= 0) st = arcs[a].x;
        rg.path[t] = a;
      }
    }
  }
  __syncthreads();
  for (int t = tid; t < T; t += NT) {
    const int a = rg.path[t];
    const int4 arc = a >= 0 ? arcs[a] : make_int4(-1, -1, 0, -1);
    pdfs[t] = arc.y;
    if (states) states[t] = arc.x;
  }
  if (states && tid == 0) states[T] = bs;
}

// align_path_labels_kernel behind align_best_path_ckpt_kernel: the chosen arc of frame t is path[t] of the utterance's region.
template <int NT>
__global__ __launch_bounds__(NT) void align_path_labels_ckpt_kernel(AlignDev g, const AlignUtt *utts, int *bp_all, const double *results,
                                                                    const int *arc_label, int *label_out, int *arc_out, int C) {
  const AlignUtt u = utts[blockIdx.y];
  const int t = blockIdx.x * NT + threadIdx.x;
  if (t >= u.frames) return;
  int arc = -1, label = -1;
  if (results[2 * (size_t)blockIdx.y + 1] != 0.0) {
    const int a = align_path_regions(bp_all, u, g.graphs[u.graph].num_states, C).path[t];
    if (a >= 0) {  // (guarded as the trace-back guards it)
      arc = g.by_dst.arcs[a].w;
      label = arc_label[arc];
    }
  }
  label_out[u.out_begin + t] = label;
  if (arc_out) arc_out[u.out_begin + t] = arc;
}

}  // namespace
}  // namespace tdnnf
