// align_compile_kernels.h -- compiles transcripts into pdf-labelled graphs on the device (align_compile.hip launches it,
// tdnnf_align_graphs_assign_transcripts asks for it): from the staged slots of a batch the raw arrays the device build
// (align_build_kernels.h) reads -- src, dst, pdf, log-prob bits, labels -- and the handle's init and final.  The graph is the one
// align_transcripts.h describes.  One launch:
//   align_compile_kernel  grid (transcripts): the workgroup walks its transcript's slots in chunks of kBuildThreads, one slot a thread.  A
//                         slot's states (A_k, and B_k behind an optional slot in context 1) and their outgoing arcs are contiguous in
//                         (source, destination) order, so the slot's first state and first arc are exclusive sums over the earlier slots:
//                         build_scan, whose carries go from chunk to chunk.  Thread 0 writes the start state and its one or two arcs.
// As the build kernels: no atomics, no workgroup waits on another, every loop's count is known at its start, plain stores, and no store
// beyond the graph's states and arcs (the host computed both from the same closed forms; the kernel checks them all the same).
#pragma once
#include "align_build_kernels.h"

namespace tdnnf {
namespace {

struct CompileOut {  // one graph's share of the arrays
  const AlignCompileDev &c;
  int s1, a1;        // one past its last state and arc
  __device__ void arc(int a, int src, int dst, int pdf, float lp, int label) const {
    if (a < 0 || a >= a1) return;  // (never: the host's closed forms are this kernel's)
    c.src[a] = src;
    c.dst[a] = dst;
    c.pdf[a] = pdf;
    c.lp_bits[a] = __float_as_int(lp);
    if (c.label) c.label[a] = label;
  }
  __device__ void state(int s, float init, float final) const {
    if (s < 0 || s >= s1) return;
    c.init[s] = init;
    c.final[s] = final;
  }
};

__device__ inline int compile_pdf_index(const AlignUnitDev &u, int left, int unit) { return u.context ? (left + 1) * u.U + unit : unit; }

__global__ __launch_bounds__(kBuildThreads) void align_compile_kernel(AlignCompileDev c) {
  __shared__ int scan[kBuildThreads];
  __shared__ int carry[2];
  const int g = blockIdx.x, tid = threadIdx.x;
  const AlignUnitDev &u = c.units;
  const int *sl = c.slots + c.slot_begin[g];
  const int n = c.slot_begin[g + 1] - c.slot_begin[g];
  const int s0 = c.state_begin[g], a0 = c.arc_begin[g];
  const CompileOut out = {c, c.state_begin[g + 1], c.arc_begin[g + 1]};
  const float ninf = -INFINITY;
  const bool start_skips = n >= 2 && (sl[0] & 1);
  if (tid == 0) {
    carry[0] = s0 + 1;
    carry[1] = a0 + (start_skips ? 2 : 1);
    out.state(s0, 0.0f, ninf);
    out.arc(a0, s0, s0 + 1, u.entry_pdf[compile_pdf_index(u, -1, sl[0] >> 1)], (sl[0] & 1) ? 0.0f + u.take_logprob : 0.0f, 0);
    if (start_skips)  // over slot 0 into slot 1: B_1 (states start, A_0, A_1, B_1) in context 1, A_1 in context 0
      out.arc(a0 + 1, s0, s0 + (u.context ? 3 : 2), u.entry_pdf[compile_pdf_index(u, -1, sl[1] >> 1)], u.skip_logprob, 1);
  }
  __syncthreads();
  for (int base = 0; base < n; base += kBuildThreads) {
    const int k = base + tid;
    const bool valid = k < n;
    // the slot, its two left neighbours (-2: unit -1, mandatory) and its two right neighbours
    const int p0 = valid ? sl[k] : 0, pm1 = valid && k >= 1 ? sl[k - 1] : -2, pm2 = valid && k >= 2 ? sl[k - 2] : -2;
    const int pp1 = k + 1 < n ? sl[k + 1] : 0, pp2 = k + 2 < n ? sl[k + 2] : 0;
    const int unit = p0 >> 1;
    const int count = valid ? 1 + (u.context && k >= 1 && (pm1 & 1) ? 1 : 0) : 0;
    const bool has_next = k + 1 < n, has_skip = k + 2 < n && (pp1 & 1);
    const int fan = 1 + (has_next ? 1 : 0) + (has_skip ? 1 : 0);
    const int sA = build_scan(count, scan, &carry[0]);
    const int aA = build_scan(count * fan, scan, &carry[1]);
    if (!valid) continue;
    const float leave = u.leave_logprob[unit], loop = u.loop_logprob[unit];
    const float fin = k == n - 1 ? leave : (k == n - 2 && (pp1 & 1)) ? leave + u.skip_logprob : ninf;
    const int next = sA + count;                                                         // A_k+1
    const int over = next + 1 + (u.context && (p0 & 1) ? 1 : 0) + (u.context ? 1 : 0);   // behind A_k+1 and B_k+1: A_k+2, or B_k+2 behind it
    const int next_pdf = has_next ? u.entry_pdf[compile_pdf_index(u, unit, pp1 >> 1)] : 0;
    const int over_pdf = has_skip ? u.entry_pdf[compile_pdf_index(u, unit, pp2 >> 1)] : 0;
    for (int i = 0; i < count; i++) {  // A_k, then B_k
      const int s = sA + i;
      int a = aA + i * fan;
      out.state(s, ninf, fin);
      out.arc(a++, s, s, u.loop_pdf[compile_pdf_index(u, (i == 0 ? pm1 : pm2) >> 1, unit)], loop, k);
      if (has_next) out.arc(a++, s, next, next_pdf, (pp1 & 1) ? leave + u.take_logprob : leave, k + 1);
      if (has_skip) out.arc(a++, s, over, over_pdf, leave + u.skip_logprob, k + 2);
    }
  }
}

}  // namespace
}  // namespace tdnnf
