// align_kernels.h -- best path (Viterbi) through cyclic, epsilon-free acceptors with pdf-ids on their arcs: forced alignment on transcript
// graphs, free decoding on the denominator graph.  Included through align_graphs.h by align.hip, which launches the kernel, and by
// align_fb.hip, which reads the same tables (AlignGraphDev, AlignDev) and constants.
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
//  * arcs: by destination, 16 bytes an arc (source state, pdf, log-prob bits, caller's arc index): one load per arc.  The states of at most
//    kAlignHeavy incoming arcs (light rows) are sorted by descending in-degree and cut into SLICES of 64, one lane each: the j-th arcs of a
//    slice's 64 rows lie side by side, so a wave's load of them is one contiguous KB (a thread per row over a CSR array touched 64 lines
//    for the same KB: with the batched loads below 46 -> 24 us per frame on the 4 000-state graph, docs/experiments.md r6-o).  Unlike the denominator's SELL-64 tables,
//    whose sums may take a row's arcs in any order, a row's arcs stay in the caller's order here (j ascending), which is what the tie rule
//    needs; a row is walked to its own length, so the padding of a slice is never read.  kAlignBatch arcs are loaded before their
//    output elements, and those before the first comparison: one round trip to the L2 per batch instead of two per arc.
//    HEAVY rows (the denominator graph of a real system has states with hundreds of incoming arcs; a slice would pad 63 rows to that
//    length) are listed per graph and taken a WAVE per row behind the light ones: the lanes stride the row's contiguous arcs, and a
//    butterfly merges the 64 partial results by (greater value, then lower position = earlier in the caller's order).
//  * gather: where two output rows of P floats fit the LDS behind the vectors and a thread can carry its share of a row in kAlignRowRegs
//    registers, the row of frame t + 1 is loaded coalesced while frame t is worked on and y[t, pdf] is an LDS read (as num_wide_kernels.h
//    gathers one frame ahead; 24 -> 10 us per frame on that graph); otherwise y[t, pdf] is a global load behind the arc's.
//  * back-pointers: bp[t * S + d] = position (in the arc table) of the arc chosen for state d at frame t + 1, or -1.
//  * trace-back: one thread walks the back-pointers from the best final state and leaves the chosen arc of frame t in bp[t * S];
//    behind a barrier the workgroup writes pdf-ids (and states) coalesced.
#pragma once
#include "common.h"

namespace tdnnf {
namespace {

constexpr int kAlignHeavy = 64;    // a state with more incoming arcs than this is a heavy row
constexpr int kAlignBatch = 4;     // arcs of a light row loaded together
constexpr int kAlignRowRegs = 8;   // floats of an output row a thread carries from one frame to the next (YLDS)

struct AlignGraphDev {  // one graph of a tdnnf_align_graphs (device table)
  int state0, num_states;  // its states are [state0, state0 + num_states) of the per-state arrays
  int slot0, num_slots;    // its light rows: slots[slot0 .. slot0 + num_slots), a multiple of 64
  int heavy0, num_heavy;   // its heavy rows: heavy[heavy0 .. heavy0 + num_heavy)
};

struct AlignUtt {  // one utterance of a call (device table at the head of the workspace)
  int graph, frames;
  int row_begin;
  int out_begin;          // first element of pdf_out; state_out starts at out_begin + (index of the utterance)
  long long bp_begin;     // first int of its back-pointers in the workspace's back-pointer region
  long long vec_begin;    // first double of its two state vectors in the workspace's vector region (global form)
};

static_assert(sizeof(AlignUtt) == 32, "the workspace formula of include/tdnnf_hip.h counts 32 bytes an utterance");

struct AlignDev {
  const AlignGraphDev *graphs;
  const int4 *slots;  // (state LOCAL to its graph or -1 for an empty lane, in-degree, position of the row's first arc: its j-th is 64 j further, 0)
  const int4 *heavy;  // (LOCAL state, first arc, one past the last arc, 0)
  const int4 *arcs;   // (source state LOCAL to its graph, pdf, log-prob bits, caller's arc index); a row's arcs in the caller's order
  const float *init, *final;  // [total states]
};

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

// grid = utterances.  LDS: the two state vectors are 2 * Smax doubles of dynamic LDS; otherwise vecs + u.vec_begin.
// YLDS (LDS only, P <= kAlignRowRegs * NT): behind the vectors the LDS holds two output rows of P floats, used alternately -- a frame's row
// is loaded coalesced one frame ahead into registers and stored to the LDS a frame later, so an arc's y[t, pdf] is an LDS read instead of a
// global load that has to wait for the arc's own load.
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
  int *bp = bp_all + u.bp_begin;
  const double scale = (double)acoustic_scale;
  float *ylds = reinterpret_cast<float *>(align_smem + 2 * (size_t)Smax);  // YLDS: two rows of P floats
  float yreg[kAlignRowRegs];
  auto row_of = [&](int t) { return y.data + (size_t)(u.row_begin + (long long)t * row_stride) * y.stride; };
  auto load_row = [&](int t) {  // (only [0, P) of a row: what the graphs' arcs can name)
    if (!YLDS || t >= T) return;
    const float *r = row_of(t);
#pragma unroll
    for (int c = 0; c < kAlignRowRegs; c++)
      if (tid + c * NT < P) yreg[c] = r[tid + c * NT];
  };
  auto store_row = [&](int t) {
    if (!YLDS || t >= T) return;
#pragma unroll
    for (int c = 0; c < kAlignRowRegs; c++)
      if (tid + c * NT < P) ylds[(size_t)(t & 1) * P + tid + c * NT] = yreg[c];
  };
  for (int s = tid; s < S; s += NT) cur[s] = (double)g.init[s0 + s];
  load_row(0);
  store_row(0);
  load_row(1);
  __syncthreads();
  for (int t = 0; t < T; t++) {
    // row t + 1 (loaded a frame ago) into the buffer whose last readers -- frame t - 1 -- are behind the previous barrier; row t + 2 on its way
    store_row(t + 1);
    load_row(t + 2);
    const float *yrow = YLDS ? ylds + (size_t)(t & 1) * P : row_of(t);
    int *bpt = bp + (size_t)t * S;
    for (int slot = tid; slot < gr.num_slots; slot += NT) {  // light rows: a lane per row, slice by slice
      const int4 row = g.slots[gr.slot0 + slot];
      if (row.x < 0) continue;
      double best = -INFINITY;
      int bi = -1;
      for (int j = 0; j < row.y; j += kAlignBatch) {
        int4 arc[kAlignBatch];
        float yv[kAlignBatch];
#pragma unroll
        for (int k = 0; k < kAlignBatch; k++) arc[k] = g.arcs[row.z + 64 * min(j + k, row.y - 1)];
#pragma unroll
        for (int k = 0; k < kAlignBatch; k++) yv[k] = yrow[arc[k].y];
#pragma unroll
        for (int k = 0; k < kAlignBatch; k++) {
          const double v = cur[arc[k].x] + ((double)__int_as_float(arc[k].z) + scale * (double)yv[k]);
          if (j + k < row.y && v > best) {
            best = v;
            bi = row.z + 64 * (j + k);
          }
        }
      }
      nxt[row.x] = best;
      bpt[row.x] = bi;
    }
    for (int h = wave; h < gr.num_heavy; h += NT / 64) {  // heavy rows: a wave per row
      const int4 row = g.heavy[gr.heavy0 + h];
      const int d = row.x;
      double best = -INFINITY;
      int bi = -1;
      for (int a = row.y + lane; a < row.z; a += 64) {
        const int4 arc = g.arcs[a];
        const double v = cur[arc.x] + ((double)__int_as_float(arc.z) + scale * (double)yrow[arc.y]);
        if (v > best) {
          best = v;
          bi = a;
        }
      }
      align_wave_best(best, bi);
      if (lane == 0) {
        nxt[d] = best;
        bpt[d] = bi;
      }
    }
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
  if (tid == 0) {  // (a reachable state at frame t + 1 has a chosen arc, whose source was reachable at frame t: no -1 on this walk; guarded all the same)
    int st = bs;
    for (int t = T - 1; t >= 0; t--) {
      const int a = bp[(size_t)t * S + st];
      if (a >= 0) st = g.arcs[a].x;
      bp[(size_t)t * S] = a;
    }
  }
  __syncthreads();
  for (int t = tid; t < T; t += NT) {
    const int a = bp[(size_t)t * S];
    const int4 arc = a >= 0 ? g.arcs[a] : make_int4(-1, -1, 0, -1);
    pdfs[t] = arc.y;
    if (states) states[t] = arc.x;
  }
  if (states && tid == 0) states[T] = bs;
}

}  // namespace
}  // namespace tdnnf
