// chain_sup_build_kernels.h -- the device build of a reserved time-synchronous tdnnf_supervision (chain_sup_build.hip launches it,
// tdnnf_supervision_assign asks for it): from the staged raw arrays of a minibatch the arc tables of chain_types.h, byte for byte what the
// host loops of tdnnf_supervision_create give.  Two launches, the second reading what the first wrote:
//   sup_build_lists_kernel   grid (sequences, 2): one workgroup builds one sequence's share of the by-destination (0) or by-source (1)
//                            lists -- the length of every state's list and every arc's place in it (original arc order: the count of
//                            earlier arcs of the sequence with the same state, build_place.h), in_begin / out_begin, and the arcs.  An arc
//                            stays inside its sequence, so the lists of sequence s begin at seq_arc_begin[s]: no offset crosses a sequence,
//                            and no workgroup needs another's result;
//   sup_build_frames_kernel  grid (sequences * frames): one wave orders the arcs that leave one frame of one sequence -- the by-source
//                            range [out_begin[fsb[t]], out_begin[fsb[t + 1]]) -- stably by pdf into pf_*: an arc's place is the number of
//                            arcs of the range with a smaller (pdf, position), counted against the range's pdfs in LDS, 64 at a time.
// Everything is in global memory (the handle's tables and scratch), so a sequence or a frame may be as large as the capacities allow; LDS
// holds a chunk's keys and a scan.  No atomics, workgroup barriers only, no workgroup waits on another, every loop's count is known at its start.
#pragma once
#include "build_place.h"

namespace tdnnf {
namespace {

constexpr int kSupFrameThreads = 64;

struct SupBuildDev {
  int B, T;
  int cap_states, cap_arcs;
  // this minibatch's raw arrays: the handle's own copies of seq_state_begin and frame_state_begin, the rest in the device staging
  const int *seq_state_begin, *seq_arc_begin, *frame_state_begin;
  const int *src, *dst, *pdf, *lp_bits;
  // the handle's tables (log-probs as their bits)
  int *begin[2];    // in_begin, out_begin
  int *other[2];    // in_src, out_dst
  int *list_pdf[2];
  int *list_lp[2];
  int *pf_src, *pf_dst, *pf_pdf, *pf_t, *pf_lp;
  // scratch: per state and table the length of its list, per arc and table its place, per by-source position its source state
  int *len[2], *arcpos[2];
  int *out_src;
};

__global__ __launch_bounds__(kBuildThreads) void sup_build_lists_kernel(SupBuildDev b) {
  __shared__ int keys[kBuildThreads];
  __shared__ int carry;
  const int s = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
  const int s0 = b.seq_state_begin[s], S = b.seq_state_begin[s + 1] - s0;
  const int a0 = b.seq_arc_begin[s], A = b.seq_arc_begin[s + 1] - a0;
  if (s0 < 0 || S < 0 || s0 + S > b.cap_states || a0 < 0 || A < 0 || a0 + A > b.cap_arcs) return;  // (never: the host validated; uniform)
  const int *key = t == 0 ? b.dst : b.src;
  int *len = b.len[t] + s0, *begin = b.begin[t] + s0, *arcpos = b.arcpos[t];

  // the lists' lengths and every arc's place in its list
  for (int r = tid; r < S; r += kBuildThreads) len[r] = 0;
  __syncthreads();
  for (int base = 0; base < A; base += kBuildThreads) {
    const int a = a0 + base + tid;
    bool valid = base + tid < A;
    const int row = valid ? key[a] - s0 : 0;
    valid = valid && row >= 0 && row < S;  // (always)
    const int place = build_stable_place(valid ? row : 0, valid, keys, len);
    if (base + tid < A) arcpos[a] = place;
  }

  // the first entry of every list: the sequence's arcs begin at a0
  if (tid == 0) carry = a0;
  __syncthreads();
  for (int base = 0; base < S; base += kBuildThreads) {
    const int r = base + tid;
    const int before = build_scan(r < S ? len[r] : 0, keys, &carry);
    if (r < S) begin[r] = before;
  }
  if (s == b.B - 1 && tid == 0) begin[S] = carry;  // (the end of the last list: the minibatch's arcs)
  __syncthreads();

  // the arcs, each to its place in its list
  for (int a = a0 + tid; a < a0 + A; a += kBuildThreads) {
    const int row = key[a] - s0;
    if (row < 0 || row >= S) continue;
    const int e = begin[row] + arcpos[a];
    if (e < a0 || e >= a0 + A) continue;
    b.other[t][e] = t == 0 ? b.src[a] : b.dst[a];
    b.list_pdf[t][e] = b.pdf[a];
    b.list_lp[t][e] = b.lp_bits[a];
    if (t == 1) b.out_src[e] = b.src[a];
  }
}

__global__ __launch_bounds__(kSupFrameThreads) void sup_build_frames_kernel(SupBuildDev b) {
  __shared__ int keys[kSupFrameThreads];
  const int s = blockIdx.x / b.T, t = blockIdx.x % b.T, tid = threadIdx.x;
  const int *fsb = b.frame_state_begin + (size_t)s * (b.T + 2);
  const int f0 = fsb[t], f1 = fsb[t + 1];
  if (f0 < 0 || f1 < f0 || f1 > b.cap_states) return;  // (never: the host validated; uniform)
  const int *out_begin = b.begin[1], *out_dst = b.other[1], *out_pdf = b.list_pdf[1], *out_lp = b.list_lp[1];
  const int o0 = out_begin[f0], n = out_begin[f1] - o0;
  if (o0 < 0 || n < 0 || o0 + n > b.cap_arcs) return;  // (never; uniform)
  for (int ibase = 0; ibase < n; ibase += kSupFrameThreads) {
    const int i = ibase + tid;
    const bool valid = i < n;
    const int mine = valid ? out_pdf[o0 + i] : 0;
    int rank = 0;
    for (int jbase = 0; jbase < n; jbase += kSupFrameThreads) {
      __syncthreads();  // (the keys of the chunk before are read)
      keys[tid] = jbase + tid < n ? out_pdf[o0 + jbase + tid] : 0;
      __syncthreads();
      const int m = min(kSupFrameThreads, n - jbase);
      for (int jj = 0; jj < m; jj++) {
        const int k = keys[jj];
        rank += (k < mine || (k == mine && jbase + jj < i)) ? 1 : 0;
      }
    }
    if (!valid) continue;
    const int e = o0 + rank;  // (rank < n: i itself is not counted)
    b.pf_src[e] = b.out_src[o0 + i];
    b.pf_dst[e] = out_dst[o0 + i];
    b.pf_pdf[e] = mine;
    b.pf_t[e] = t;
    b.pf_lp[e] = out_lp[o0 + i];
  }
}

}  // namespace
}  // namespace tdnnf
