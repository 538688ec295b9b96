// chain_sup_compile_kernels.h -- compiles alignments and a frame tolerance into time-synchronous supervision lattices on the device
// (chain_sup_compile.hip launches it; tdnnf_supervision_assign_alignments and tdnnf_supervision_assign_alignment_chunks ask for it): from
// the staged units and entry windows of a minibatch the raw arrays the device build (chain_sup_build_kernels.h) reads -- src, dst, pdf,
// log-prob bits, in (source, destination) order -- and the supervision's state_time and final_logprob.  The lattice, the closed form of a
// frame and what one state writes (ali_chunk_state, which a host test runs too) are chain_sup_alignment.h's.  A sequence is a chunk of an
// utterance's lattice, the frames [o, o + T) behind a start of its own; a whole alignment is the chunk o = 0 of an utterance of T frames.
// One launch:
//   sup_compile_kernel  grid (sequences): the workgroup first gives every frame 0 .. T of its sequence the index of the first arc that
//                       leaves it -- a frame's arcs from AliFrame at the time o + t, two binary searches on the staged windows a frame,
//                       summed by build_scan with the carry from one block of frames to the next -- into the build's scratch; then it walks
//                       the sequence's states, one a thread: the state's frame by a binary search on frame_state_begin, its unit from the
//                       frame's E and L blocks, its first arc from the frame's plus the arcs of the states before it in the frame
//                       (AliFrame::degsum), its one or two destinations from the blocks of the next frame.  The start's arcs, one into
//                       every state of time 1, are written from their destinations: the j-th state of time 1 stores arc j of the
//                       sequence, so no thread loops over a frame's width.  Every state of time T is final.  Stores go out in state order.
// As the build kernels: no atomics, workgroup barriers only, no workgroup waits on another, every loop's count is known at its start, plain
// stores, and no store beyond the sequence's states and arcs (the host computed both from the same closed form; the kernel checks them all
// the same).
#pragma once
#include "build_place.h"
#include "chain_sup_alignment.h"

namespace tdnnf {
namespace {

struct SupCompileOut {  // one sequence's share of the arrays
  const SupCompileDev &c;
  int s0, s1, a0, a1;
  __device__ void arc(int a, int src, int dst, int pdf) const {
    if (a < a0 || a >= a1 || dst < s0 || dst >= s1) return;  // (never: the host's closed form is this kernel's)
    c.src[a] = src;
    c.dst[a] = dst;
    c.pdf[a] = pdf;
    c.lp_bits[a] = 0;  // (the bits of 0.0f: the lattice is unweighted)
  }
};

__device__ inline int sup_compile_pdf_index(const AlignUnitDev &u, int left, int unit) { return u.context ? (left + 1) * u.U + unit : unit; }

__global__ __launch_bounds__(kBuildThreads) void sup_compile_kernel(SupCompileDev c) {
  __shared__ int scan[kBuildThreads];
  __shared__ int carry;
  const int s = blockIdx.x, tid = threadIdx.x, T = c.T;
  const AlignUnitDev &u = c.units_dev;
  const int q0 = c.slice_begin[s], cnt = c.slice_begin[s + 1] - q0;
  const int s0 = c.seq_state_begin[s], S = c.seq_state_begin[s + 1] - s0;
  const int a0 = c.seq_arc_begin[s], a1 = c.seq_arc_begin[s + 1];
  const int *ck = c.chunk ? c.chunk + 4 * (size_t)s : nullptr;
  const int Tu = ck ? ck[0] : T, n = ck ? ck[1] : cnt, o = ck ? ck[2] : 0, base = ck ? ck[3] : 0;
  // (never: the host validated and planned; uniform.  A sequence has a state of every time 0 .. T)
  if (q0 < 0 || cnt < 1 || s0 < 0 || S < T + 1 || s0 + S > c.cap_states || a0 < 0 || a1 < a0 || a1 > c.cap_arcs) return;
  if (base < 0 || (long long)base + cnt > n || o < 0 || (long long)o + T > Tu) return;
  // the staged slice by the unit's number in the utterance: only [base, base + cnt) is read
  const AliChunk ch = {c.units + q0 - base, c.lo + q0 - base, c.hi + q0 - base, n, Tu, o, T, base, cnt};
  const int *fsb = c.frame_state_begin + (size_t)s * (T + 2);
  int *fab = c.frame_arc_begin + s0;
  const SupCompileOut out = {c, s0, s0 + S, a0, a1};

  // the first arc that leaves every frame
  if (tid == 0) carry = a0;
  __syncthreads();
  for (int first = 0; first <= T; first += kBuildThreads) {
    const int t = first + tid;
    const int before = build_scan(t <= T ? ali_chunk_frame_arcs(ch, t) : 0, scan, &carry);
    if (t <= T) fab[t] = before;
  }
  __syncthreads();

  // the states and their arcs
  for (int i = tid; i < S; i += kBuildThreads) {
    const int g = s0 + i;
    const AliState st = ali_chunk_state(ch, fsb, fab, s0, a0, g);
    if (st.t < 0) continue;  // (never)
    c.state_time[g] = st.t;
    c.final_logprob[g] = st.t == T ? 0.0f : -INFINITY;
#pragma unroll
    for (int q = 0; q < 3; q++)
      if (st.arc[q].a >= 0) {
        const AliArc &r = st.arc[q];
        const int at = sup_compile_pdf_index(u, r.left, r.unit);
        out.arc(r.a, r.src, r.dst, r.entry ? u.entry_pdf[at] : u.loop_pdf[at]);
      }
  }
}

}  // namespace
}  // namespace tdnnf
