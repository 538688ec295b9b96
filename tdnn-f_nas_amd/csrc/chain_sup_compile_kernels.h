// chain_sup_compile_kernels.h -- compiles alignments and a frame tolerance into time-synchronous supervision lattices on the device
// (chain_sup_compile.hip launches it, tdnnf_supervision_assign_alignments asks for it): from the staged units and entry windows of a
// minibatch the raw arrays the device build (chain_sup_build_kernels.h) reads -- src, dst, pdf, log-prob bits, in (source, destination)
// order -- and the supervision's state_time and final_logprob.  The lattice and the closed form of a frame are chain_sup_alignment.h's.
// One launch:
//   sup_compile_kernel  grid (sequences): the workgroup first gives every frame 0 .. T of its sequence the index of the first arc that
//                       leaves it -- a frame's arcs from AliFrame, two binary searches on the windows a frame, summed by build_scan with the
//                       carry from chunk to chunk -- into the build's scratch; then it walks the sequence's states, one a thread: the state's
//                       frame by a binary search on frame_state_begin, its unit from the frame's E and L blocks, its first arc from the
//                       frame's plus the arcs of the states before it in the frame (AliFrame::degsum), its one or two destinations from the
//                       blocks of the next frame.  Stores go out in state order.
// As the build kernels: no atomics, workgroup barriers only, no workgroup waits on another, every loop's count is known at its start, plain
// stores, and no store beyond the sequence's states and arcs (the host computed both from the same closed form; the kernel checks them all
// the same).
#pragma once
#include "build_place.h"
#include "chain_sup_alignment.h"

namespace tdnnf {
namespace {

__device__ inline int sup_count_le(const int *v, int n, int x) {  // #{k < n: v[k] <= x}, v ascending
  int a = 0, b = n;
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (v[mid] <= x) a = mid + 1; else b = mid;
  }
  return a;
}

__device__ inline AliFrame sup_frame_at(const int *lo, const int *hi, int n, int T, int t) {
  return ali_frame(lo, hi, n, T, t, sup_count_le(lo, n, t - 2), sup_count_le(hi, n, t - 2));  // (#{hi < t - 1}: integers)
}

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
  const int k0 = c.unit_begin[s], n = c.unit_begin[s + 1] - k0;
  const int s0 = c.seq_state_begin[s], S = c.seq_state_begin[s + 1] - s0;
  const int a0 = c.seq_arc_begin[s], a1 = c.seq_arc_begin[s + 1];
  // (never: the host validated and planned; uniform.  A sequence has a state of every time 0 .. T)
  if (k0 < 0 || n < 1 || s0 < 0 || S < T + 1 || s0 + S > c.cap_states || a0 < 0 || a1 < a0 || a1 > c.cap_arcs) return;
  const int *unit = c.units + k0, *lo = c.lo + k0, *hi = c.hi + k0;
  const int *fsb = c.frame_state_begin + (size_t)s * (T + 2);
  int *fab = c.frame_arc_begin + s0;
  const SupCompileOut out = {c, s0, s0 + S, a0, a1};

  // the first arc that leaves every frame
  if (tid == 0) carry = a0;
  __syncthreads();
  for (int base = 0; base <= T; base += kBuildThreads) {
    const int t = base + tid;
    const int arcs = t == 0 ? 1 : t <= T ? sup_frame_at(lo, hi, n, T, t).arcs() : 0;
    const int before = build_scan(arcs, scan, &carry);
    if (t <= T) fab[t] = before;
  }
  __syncthreads();

  // the states and their arcs
  const float ninf = -INFINITY;
  for (int i = tid; i < S; i += kBuildThreads) {
    const int g = s0 + i;
    int t = 0, b = T;  // the last frame that begins at or before the state
    while (t < b) {
      const int mid = (t + b + 1) >> 1;
      if (fsb[mid] <= g) t = mid; else b = mid - 1;
    }
    if (t == 0) {
      if (i != 0) continue;  // (never: one state of time 0)
      c.state_time[g] = 0;
      c.final_logprob[g] = ninf;
      out.arc(a0, g, s0 + 1, u.entry_pdf[sup_compile_pdf_index(u, -1, unit[0])]);
      continue;
    }
    const AliFrame f = sup_frame_at(lo, hi, n, T, t);
    const int j = g - fsb[t];
    if (j < 0 || j >= f.states()) continue;  // (never)
    const bool entered = j < f.nE;
    const int k = entered ? f.kE0 + j : f.kL0 + (j - f.nE);
    if (k < 0 || k >= n) continue;  // (never)
    c.state_time[g] = t;
    c.final_logprob[g] = t == T && k == n - 1 ? 0.0f : ninf;
    if (t == T) continue;
    int a = fab[t] + (entered ? f.degsum(f.kE0, j) : f.degsum(f.kE0, f.nE) + f.degsum(f.kL0, j - f.nE));
    const AliFrame f1 = ali_frame(lo, hi, n, T, t + 1, f.a1, f.h0);
    const int next = fsb[t + 1];
    if (f.enters(k)) out.arc(a++, g, next + (k + 1 - f1.kE0), u.entry_pdf[sup_compile_pdf_index(u, unit[k], unit[k + 1])]);
    if (f.stays(k)) out.arc(a++, g, next + f1.nE + (k - f1.kL0), u.loop_pdf[sup_compile_pdf_index(u, k > 0 ? unit[k - 1] : -1, unit[k])]);
  }
}

}  // namespace
}  // namespace tdnnf
