// align_pron_compile_kernels.h -- compiles transcripts with pronunciation alternatives into pdf-labelled graphs on the device
// (align_pron_compile.hip launches it, tdnnf_align_graphs_assign_pronunciations asks for it): from the staged tables of a batch the raw
// arrays the device build (align_build_kernels.h) reads -- src, dst, pdf, log-prob bits, labels -- and the handle's init and final.  The
// graph is the one align_pronunciations.h describes.  One launch:
//   align_pron_compile_kernel  grid (transcripts): the workgroup walks its transcript's entries in chunks of kBuildThreads, one entry a
//                              thread.  An entry's states and their outgoing arcs are contiguous in (source, destination) order, so the
//                              entry's first state and first arc are exclusive sums over the earlier entries: build_scan, whose carries go
//                              from chunk to chunk.  Where an arc ENTERS is no sum of what lies before its source: the first state of a
//                              position comes staged from the host's closed forms (pos_info), an alternative's follows from it.  The
//                              start's arcs go round the threads in front of the first chunk.
// As the build kernels: no atomics, no workgroup waits on another, every loop's count is known at its start, plain stores, and no store
// beyond the graph's states and arcs (the host computed both from the same closed forms; the kernel checks them all the same).
#pragma once
#include "align_compile_kernels.h"

namespace tdnnf {
namespace {

struct PronGraph {  // one transcript's tables; positions and alternatives by their index in the batch
  const AlignPronCompileDev &c;
  int P0, n;  // its first position, their number
  int e0;     // its first entry
  __device__ int alts(int P) const { return c.pos_alt_begin[P + 1] - c.pos_alt_begin[P]; }
  __device__ bool optional(int P) const { return c.pos_info[P] & 1; }
  // the predecessors of position P: the alternatives of P - 1 (the start in front of the first position), and behind an optional P - 1 those of P - 2
  __device__ int near(int P) const { return P == P0 ? 1 : alts(P - 1); }
  __device__ int far(int P) const { return P > P0 && optional(P - 1) ? (P == P0 + 1 ? 1 : alts(P - 2)) : 0; }
  __device__ int first_states(int P) const { return c.units.context ? near(P) + far(P) : 1; }  // N_p: of a first entry
  // the first state of alternative q of position P, local to the graph: every alternative before it has N_p + L - 1 states
  __device__ int alt_state(int P, int q) const {
    const int qb = c.pos_alt_begin[P];
    return (c.pos_info[P] >> 1) + (q - qb) * (first_states(P) - 1) + (c.alt_unit_begin[q] - c.alt_unit_begin[qb]);
  }
  __device__ int last_unit(int q) const { return c.alt_units[c.alt_unit_begin[q + 1] - 1]; }
  __device__ int first_unit(int q) const { return c.alt_units[c.alt_unit_begin[q]]; }
};

// One arc out of state s (unit `unit`, or -1: the start) into the first entry of alternative q of position P, into that entry's state number
// `mine`; base: the weight so far.
__device__ inline void pron_enter(const CompileOut &out, const PronGraph &t, int s0, int a, int s, int unit, int P, int q, int mine, float base) {
  const AlignUnitDev &u = t.c.units;
  const float w = t.alts(P) >= 2 ? base + t.c.alt_logprob[q] : base;
  out.arc(a, s, s0 + t.alt_state(P, q) + mine, u.entry_pdf[compile_pdf_index(u, unit, t.first_unit(q))], w, t.c.alt_unit_begin[q] - t.e0);
}

__global__ __launch_bounds__(kBuildThreads) void align_pron_compile_kernel(AlignPronCompileDev c) {
  __shared__ int scan[kBuildThreads];
  __shared__ int carry[2];
  const int g = blockIdx.x, tid = threadIdx.x;
  const AlignUnitDev &u = c.units;
  const int P0 = c.pos_begin[g], n = c.pos_begin[g + 1] - P0;
  const int q0 = c.pos_alt_begin[P0], q1 = c.pos_alt_begin[P0 + n];
  const int e0 = c.alt_unit_begin[q0], E = c.alt_unit_begin[q1] - e0;
  const PronGraph t = {c, P0, n, e0};
  const int s0 = c.state_begin[g], a0 = c.arc_begin[g];
  const AlignCompileDev arrays = {nullptr, nullptr, nullptr, nullptr, c.src, c.dst, c.pdf, c.lp_bits, c.label, c.init, c.final, u};  // (what CompileOut writes)
  const CompileOut out = {arrays, c.state_begin[g + 1], c.arc_begin[g + 1]};
  const float ninf = -INFINITY;
  // the start: the last entry of a position in front of the first, with no leave term
  const int start_near = t.alts(P0), start_far = n >= 2 && t.optional(P0) ? t.alts(P0 + 1) : 0;
  if (tid == 0) {
    carry[0] = s0 + 1;
    carry[1] = a0 + start_near + start_far;
    out.state(s0, 0.0f, ninf);
  }
  for (int i = tid; i < start_near + start_far; i += kBuildThreads) {
    if (i < start_near)
      pron_enter(out, t, s0, a0 + i, s0, -1, P0, q0 + i, 0, t.optional(P0) ? 0.0f + u.take_logprob : 0.0f);
    else  // over position 0: the start is position 1's one far predecessor, behind its near ones
      pron_enter(out, t, s0, a0 + i, s0, -1, P0 + 1, c.pos_alt_begin[P0 + 1] + i - start_near, u.context ? start_near : 0, u.skip_logprob);
  }
  __syncthreads();
  for (int base = 0; base < E; base += kBuildThreads) {
    const int k = base + tid;  // the entry's number in its transcript
    const bool valid = k < E;
    int q = q0;
    if (valid) {  // its alternative: the last whose first entry is not behind it
      int lo = q0, hi = q1 - 1;
      while (lo < hi) {  // (at most 31 halvings)
        const int mid = (lo + hi + 1) >> 1;
        if (c.alt_unit_begin[mid] <= e0 + k) lo = mid; else hi = mid - 1;
      }
      q = lo;
    }
    const int P = c.alt_pos[q], p = P - P0;
    const int j = e0 + k - c.alt_unit_begin[q], L = c.alt_unit_begin[q + 1] - c.alt_unit_begin[q];
    const bool is_last = j == L - 1;
    const int unit = valid ? c.alt_units[e0 + k] : 0;
    const int near = t.near(P);
    const int count = valid ? (j == 0 ? t.first_states(P) : 1) : 0;
    // a last entry's arcs into position p + 1 and, over an optional position p + 1, into position p + 2
    const int into_next = is_last && p + 1 < n ? t.alts(P + 1) : 0;
    const int into_over = is_last && p + 2 < n && t.optional(P + 1) ? t.alts(P + 2) : 0;
    const int fan = 1 + (is_last ? into_next + into_over : 1);
    const int sA = build_scan(count, scan, &carry[0]);
    const int aA = build_scan(count * fan, scan, &carry[1]);
    if (!valid) continue;
    const float leave = u.leave_logprob[unit], loop = u.loop_logprob[unit];
    const float fin = !is_last ? ninf : p == n - 1 ? leave : (p == n - 2 && t.optional(P + 1)) ? leave + u.skip_logprob : ninf;
    const int a_of = q - c.pos_alt_begin[P];  // this alternative among its position's: its place among the near predecessors of p + 1
    const int next_pdf = is_last ? 0 : u.entry_pdf[compile_pdf_index(u, unit, c.alt_units[e0 + k + 1])];
    const float enter_w = into_next && t.optional(P + 1) ? leave + u.take_logprob : leave;
    for (int i = 0; i < count; i++) {  // a first entry's states: the near predecessors, then the far ones
      const int s = sA + i;
      int a = aA + i * fan;
      int left = -1;
      if (j > 0)
        left = c.alt_units[e0 + k - 1];
      else if (u.context && i < near)
        left = p == 0 ? -1 : t.last_unit(c.pos_alt_begin[P - 1] + i);
      else if (u.context)
        left = p == 1 ? -1 : t.last_unit(c.pos_alt_begin[P - 2] + i - near);
      out.state(s, ninf, fin);
      out.arc(a++, s, s, u.loop_pdf[compile_pdf_index(u, left, unit)], loop, k);
      if (!is_last) out.arc(a++, s, sA + count, next_pdf, leave, k + 1);
      for (int x = 0; x < into_next; x++) pron_enter(out, t, s0, a++, s, unit, P + 1, c.pos_alt_begin[P + 1] + x, u.context ? a_of : 0, enter_w);
      for (int x = 0; x < into_over; x++)  // the far predecessors of p + 2 stand behind its near ones, the alternatives of p + 1
        pron_enter(out, t, s0, a++, s, unit, P + 2, c.pos_alt_begin[P + 2] + x, u.context ? into_next + a_of : 0, leave + u.skip_logprob);
    }
  }
}

}  // namespace
}  // namespace tdnnf
