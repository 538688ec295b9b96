// chain_sup_alignment.h -- the host side of compiling a time-synchronous supervision from alignments and a frame tolerance
// (include/tdnnf_hip.h, "ALIGNMENT SUPERVISIONS"; tdnnf_supervision_assign_alignments, tdnnf_alignment_supervision_sizes): the validation of
// a minibatch of (unit, start frame) sequences, the entry windows of every unit, and everything the assign records and stages of the
// lattice -- the whole SupPlan of chain_sup_tables.h, seq_state_begin and seq_arc_begin -- from the closed form of a frame, without holding
// a state or an arc: O(units + B * (T + 2)).  The kernel that writes the states and arcs (chain_sup_compile_kernels.h) evaluates the same
// closed form, AliFrame below.  Plain C++ with no device header, so that a test builds it with g++ (tests/alignment_driver.cc under the
// address and undefined-behaviour sanitizers, tests/test_alignment_plan_cpu.py).
//
// The lattice of one sequence (T frames, units u_0 .. u_n-1 starting at b_0 = 0 < b_1 < ... < T, windows lo_k <= b_k <= hi_k, both strictly
// increasing, lo_n = hi_n = T): the start; E(t, k) for lo_k + 1 <= t <= hi_k + 1 (unit k entered at frame t - 1); L(t, k) for
// lo_k + 2 <= t <= hi_k+1 (frame t - 1 was a later frame of unit k).  Within one time all E by k, then all L by k.  From X(t, k) the enter
// arc to E(t + 1, k + 1) if k + 1 < n and lo_k+1 <= t <= hi_k+1, then the stay arc to L(t + 1, k) if t + 1 <= hi_k+1.  With
//   A(x) = #{k < n: lo_k <= x}   and   H(x) = #{k < n: hi_k < x}
// the E states of time t are the units [H(t - 1), A(t - 1)), the L states the units [H(t) - 1, A(t - 2)); every state of time t has
// hi_k+1 >= t, so the only unit that cannot stay is the one with hi_k+1 = t (k = H(t) - 1, if at all), and "can enter k + 1" is k + 1 < A(t).
#pragma once
#include <stdio.h>

#include <string>
#include <vector>

#include "align_transcripts.h"
#include "chain_sup_tables.h"

#ifdef __HIP__
#define TDNNF_ALI_HD __host__ __device__
#else
#define TDNNF_ALI_HD
#endif

namespace tdnnf {

struct AliFrame {  // the states of one time t >= 1 of one sequence, and their arcs
  int kE0, nE;     // E(t, k) for k in [kE0, kE0 + nE)
  int kL0, nL;     // L(t, k) for k in [kL0, kL0 + nL), behind the E states
  int kstar;       // the one unit whose states of this time have no stay arc, or -1
  int m;           // A(t): the states of unit k have an enter arc iff k + 1 < m
  int a1, h0;      // A(t - 1) and H(t): what the frame t + 1 starts from
  TDNNF_ALI_HD int states() const { return nE + nL; }
  // the arcs that leave the c states of units a .. a + c - 1 (one block of the frame)
  TDNNF_ALI_HD int degsum(int a, int c) const {
    const int enter = m - 1 - a < 0 ? 0 : m - 1 - a > c ? c : m - 1 - a;
    return c - (kstar >= a && kstar < a + c ? 1 : 0) + enter;
  }
  TDNNF_ALI_HD bool stays(int k) const { return k != kstar; }
  TDNNF_ALI_HD bool enters(int k) const { return k + 1 < m; }
  TDNNF_ALI_HD int arcs() const { return degsum(kE0, nE) + degsum(kL0, nL); }
};

// The frame t in [1, T] of a sequence with the windows lo / hi [n] from a2 = A(t - 2) and h1 = H(t - 1): both windows increase strictly,
// so each count moves by one at most from a frame to the next.
TDNNF_ALI_HD inline AliFrame ali_frame(const int *lo, const int *hi, int n, int T, int t, int a2, int h1) {
  AliFrame f;
  f.a1 = a2 + (a2 < n && lo[a2] == t - 1 ? 1 : 0);
  f.m = f.a1 + (f.a1 < n && lo[f.a1] == t ? 1 : 0);
  f.h0 = h1 + (h1 < n && hi[h1] == t - 1 ? 1 : 0);
  f.kE0 = h1;
  f.nE = f.a1 - h1;
  f.kL0 = f.h0 - 1;
  f.nL = a2 - f.kL0 > 0 ? a2 - f.kL0 : 0;
  f.kstar = (f.h0 < n ? hi[f.h0] : T) == t ? f.h0 - 1 : -1;
  return f;
}

inline std::string alignment_message(const char *fmt, const char *who, int a = 0, int b = 0, int c = 0, int d = 0) {
  char buf[512];
  snprintf(buf, sizeof(buf), fmt, who, a, b, c, d);
  return buf;
}

// What every entry that takes alignments refuses; false with *err set.  who: the prefix of the messages, the call's name.
inline bool alignments_validate(const char *who, const TranscriptUnits &u, int B, int T, const int *unit_begin, const int *units, const int *starts,
                                int tolerance, std::string *err) {
  if (B <= 0 || T <= 0 || !unit_begin || !units || !starts) {
    *err = alignment_message("%sbad arguments (num_sequences %d, frames_per_sequence %d, or a null array)", who, B, T);
    return false;
  }
  if (tolerance < 0) {
    *err = alignment_message("%stolerance %d is negative", who, tolerance);
    return false;
  }
  if (unit_begin[0] != 0) {
    *err = alignment_message("%sunit_begin must start at 0", who);
    return false;
  }
  for (int s = 0; s < B; s++) {
    const int k0 = unit_begin[s], n = unit_begin[s + 1] - k0;
    if (n < 1) {
      *err = alignment_message("%ssequence %d has %d units: an alignment has one at least (unit_begin must not decrease)", who, s, n);
      return false;
    }
    for (int k = 0; k < n; k++) {
      const int b = starts[k0 + k];
      if (units[k0 + k] < 0 || units[k0 + k] >= u.U) {
        *err = alignment_message("%ssequence %d unit %d: unit %d outside [0, %d)", who, s, k, units[k0 + k], u.U);
        return false;
      }
      if (k == 0 && b != 0) {
        *err = alignment_message("%ssequence %d unit 0: starts at frame %d, the first unit starts at frame 0", who, s, b);
        return false;
      }
      if (k > 0 && b <= starts[k0 + k - 1]) {
        *err = alignment_message("%ssequence %d unit %d: starts at frame %d, not behind the start %d of the unit before it", who, s, k, b, starts[k0 + k - 1]);
        return false;
      }
      if (b >= T) {
        *err = alignment_message("%ssequence %d unit %d: starts at frame %d, outside the %d frames of a sequence", who, s, k, b, T);
        return false;
      }
    }
  }
  return true;
}

// The entry windows of one validated sequence: lo / hi [n].
inline void alignment_windows(int n, int T, const int *starts, int tolerance, int *lo, int *hi) {
  const int tol = std::min(tolerance, T);  // (the windows are cut to [0, T - 1] anyway; no sum overflows)
  for (int k = 0; k < n; k++) {
    lo[k] = std::max(starts[k] - tol, 0);
    hi[k] = std::min(starts[k] + tol, T - 1);
  }
  lo[0] = hi[0] = 0;
  for (int k = 1; k < n; k++) lo[k] = std::max(lo[k], lo[k - 1] + 1);
  for (int k = n - 1, next = T; k >= 0; k--) next = hi[k] = std::min(hi[k], next - 1);
}

struct AlignmentSupPlan {  // a validated minibatch as tdnnf_supervision_assign_alignments stages and records it
  SupPlan plan;
  std::vector<int> seq_state_begin, seq_arc_begin;  // [B + 1]
  std::vector<int> lo, hi;                          // [units]: what the kernel reads beside the units
};

// Plans a minibatch that alignments_validate accepted: what sup_validate and sup_widths find on the lattice's arrays, from the frames'
// closed form.  False with *err set: 2^31 states or arcs, or more.
inline bool alignments_plan(const char *who, int B, int T, const int *unit_begin, const int *starts, int tolerance, AlignmentSupPlan *ap,
                            std::string *err) {
  SupPlan &p = ap->plan;
  p.max_states_per_seq = p.max_states_per_frame = p.max_arcs_per_frame = p.max_arcs_per_seq = 0;
  p.frame_state_begin.assign((size_t)B * (T + 2), 0);
  ap->seq_state_begin.assign(1, 0);
  ap->seq_arc_begin.assign(1, 0);
  ap->lo.resize(unit_begin[B]);
  ap->hi.resize(unit_begin[B]);
  long long NS = 0, NA = 0;
  for (int s = 0; s < B; s++) {
    const int k0 = unit_begin[s], n = unit_begin[s + 1] - k0;
    int *lo = ap->lo.data() + k0, *hi = ap->hi.data() + k0;
    alignment_windows(n, T, starts + k0, tolerance, lo, hi);
    int *fsb = p.frame_state_begin.data() + (size_t)s * (T + 2);
    long long S = 1, A = 1;  // the start and its arc into E(1, 0)
    fsb[0] = (int)NS;
    p.max_states_per_frame = std::max(p.max_states_per_frame, 1);
    p.max_arcs_per_frame = std::max(p.max_arcs_per_frame, 1);
    int a2 = 0, h1 = 0;
    for (int t = 1; t <= T; t++) {
      const AliFrame f = ali_frame(lo, hi, n, T, t, a2, h1);
      if (NS + S >= (1ll << 31) || NA + A >= (1ll << 31)) break;
      fsb[t] = (int)(NS + S);
      S += f.states();
      A += f.arcs();
      p.max_states_per_frame = std::max(p.max_states_per_frame, f.states());
      p.max_arcs_per_frame = std::max(p.max_arcs_per_frame, f.arcs());
      a2 = f.a1;
      h1 = f.h0;
    }
    NS += S;
    NA += A;
    if (NS >= (1ll << 31) || NA >= (1ll << 31)) {
      *err = alignment_message("%sthe minibatch has more than 2^31 states or arcs (at sequence %d)", who, s);
      return false;
    }
    fsb[T + 1] = (int)NS;
    p.max_states_per_seq = std::max(p.max_states_per_seq, (int)S);
    p.max_arcs_per_seq = std::max(p.max_arcs_per_seq, (int)A);
    ap->seq_state_begin.push_back((int)NS);
    ap->seq_arc_begin.push_back((int)NA);
  }
  p.num_states = (int)NS;
  p.num_arcs = (int)NA;
  p.wide = (long long)p.num_states > (long long)B * 4 * (T + 1);
  return true;
}

// tdnnf_alignment_supervision_sizes but for the handle: the states and arcs of every sequence's lattice (either out-pointer may be null),
// refusing what the assign refuses.
inline bool alignment_sizes(const char *who, const TranscriptUnits &u, int B, int T, const int *unit_begin, const int *units, const int *starts,
                            int tolerance, int *states_out, int *arcs_out, std::string *err) {
  AlignmentSupPlan ap;
  if (!alignments_validate(who, u, B, T, unit_begin, units, starts, tolerance, err) || !alignments_plan(who, B, T, unit_begin, starts, tolerance, &ap, err))
    return false;
  for (int s = 0; s < B; s++) {
    if (states_out) states_out[s] = ap.seq_state_begin[s + 1] - ap.seq_state_begin[s];
    if (arcs_out) arcs_out[s] = ap.seq_arc_begin[s + 1] - ap.seq_arc_begin[s];
  }
  return true;
}

}  // namespace tdnnf

#ifdef __HIP__  // (the compiler's own mark of a .hip file: g++ sees the plain half only)
#include "align_graphs.h"

namespace tdnnf {

// What the compile kernel (chain_sup_compile_kernels.h) takes by value; chain_sup_compile.hip launches it.
struct SupCompileDev {
  int B, T;
  int cap_states, cap_arcs;
  const int *unit_begin, *seq_arc_begin;            // [B + 1] (device staging)
  const int *units, *lo, *hi;                       // [units] (device staging)
  const int *seq_state_begin, *frame_state_begin;   // the supervision's own arrays, copied in front of the launch
  int *state_time;                                  // [states] the supervision's
  float *final_logprob;                             // [states] the supervision's
  int *src, *dst, *pdf, *lp_bits;                   // [arcs] device staging: what SupBuildDev reads
  int *frame_arc_begin;                             // the build's scratch (its by-destination lengths, one int a state: a sequence has more
                                                    // states than frames): sequence s's frames 0 .. T at seq_state_begin[s] + t
  AlignUnitDev units_dev;
};

int sup_compile_launch(const SupCompileDev &c, hipStream_t s);

}  // namespace tdnnf
#endif
