// chain_sup_alignment.h -- the host side of compiling a time-synchronous supervision from alignments and a frame tolerance
// (include/tdnnf_hip.h, "ALIGNMENT SUPERVISIONS"; tdnnf_supervision_assign_alignments, tdnnf_alignment_supervision_sizes): the validation of
// a minibatch of (unit, start frame) sequences, the entry windows of every unit, and everything the assign records and stages of the
// lattice -- the whole SupPlan of chain_sup_tables.h, seq_state_begin and seq_arc_begin -- from the closed form of a frame, without holding
// a state or an arc: O(units + B * (T + 2)).  The kernel that writes the states and arcs (chain_sup_compile_kernels.h) evaluates the same
// closed form, AliFrame below.  Plain C++ with no device header, so that a test builds it with g++ (tests/alignment_driver.cc under the
// address and undefined-behaviour sanitizers, tests/test_alignment_plan_cpu.py).
// A CHUNK (include/tdnnf_hip.h, "ALIGNMENT CHUNKS"; tdnnf_supervision_assign_alignment_chunks, tdnnf_alignment_chunk_supervision_sizes) is
// the window [o + 1, o + T] of the times of an utterance's lattice behind a start of its own: the same closed form at the absolute time
// o + t, over the slice of the utterance's units that those times can name (AliChunk below).  A whole alignment is the chunk o = 0,
// T = the utterance's frames, its slice every unit; one plan (alignment_chunks_plan) and one kernel serve both, and
// tests/alignment_chunk_driver.cc runs the kernel's own per-state function (ali_chunk_state) on the host against the lattice's arrays.
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

#include <algorithm>
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

// One sequence as the compile kernel sees it: the frames [o, o + T) of an utterance of Tu frames and n units, of which the units
// [base, base + cnt) are staged -- unit, lo and hi are indexed by the unit's number in the utterance and hold those alone.  The slice is
// what alignment_chunks_plan chose: every count A(x), x in [o - 1, o + T], and H(x), x in [o, o + T], is base + the count over the slice,
// and every unit a state or an arc of the times [o + 1, o + T] names, with its left neighbour, is inside.
struct AliChunk {
  const int *unit, *lo, *hi;
  int n, Tu, o, T, base, cnt;
};

TDNNF_ALI_HD inline int ali_count_le(const int *v, int n, int x) {  // #{k < n: v[k] <= x}, v ascending
  int a = 0, b = n;
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (v[mid] <= x) a = mid + 1; else b = mid;
  }
  return a;
}

// The frame t in [1, T] of a chunk: the utterance's at the time o + t, from two binary searches on the slice.
TDNNF_ALI_HD inline AliFrame ali_chunk_frame(const AliChunk &c, int t) {
  const int x = c.o + t - 2;  // A(x), and H(x + 1) = #{hi <= x}: integers
  return ali_frame(c.lo, c.hi, c.n, c.Tu, c.o + t, c.base + ali_count_le(c.lo + c.base, c.cnt, x), c.base + ali_count_le(c.hi + c.base, c.cnt, x));
}

// The arcs that leave the frame t in [0, T] of a chunk: one from the start to every state of time 1, none out of the last frame.
TDNNF_ALI_HD inline int ali_chunk_frame_arcs(const AliChunk &c, int t) {
  return t == 0 ? ali_chunk_frame(c, 1).states() : t < c.T ? ali_chunk_frame(c, t).arcs() : 0;
}

struct AliArc {  // arc number `a` from src to dst with the entry (else the loop) pdf at (left, unit); left -1: nothing before it
  int a, src, dst, left, unit;
  bool entry;
};

struct AliState {  // what the thread of one state writes: its time, and its arcs
  int t;           // -1: not a state of the sequence (never for planned arrays)
  AliArc arc[3];   // for a state of time 1 the start's arc into it, the state's own enter arc, its stay arc; a < 0: none
};

// State g of a chunk whose states begin at s0 and whose arcs at a0.  fsb: the sequence's frame_state_begin [T + 2]; fab [T + 1]: the first
// arc that leaves every frame (a0 + the running sum of ali_chunk_frame_arcs).
TDNNF_ALI_HD inline AliState ali_chunk_state(const AliChunk &c, const int *fsb, const int *fab, int s0, int a0, int g) {
  AliState st;
  st.t = -1;
  st.arc[0].a = st.arc[1].a = st.arc[2].a = -1;
  int t = 0, b = c.T;  // the last frame that begins at or before the state
  while (t < b) {
    const int mid = (t + b + 1) >> 1;
    if (fsb[mid] <= g) t = mid; else b = mid - 1;
  }
  if (t == 0) {
    if (g == s0) st.t = 0;  // (the start: its arcs are written by the states of time 1)
    return st;
  }
  const AliFrame f = ali_chunk_frame(c, t);
  const int j = g - fsb[t];
  if (j < 0 || j >= f.states()) return st;
  const bool entered = j < f.nE;
  const int k = entered ? f.kE0 + j : f.kL0 + (j - f.nE);
  if (k < c.base || k >= c.base + c.cnt) return st;
  st.t = t;
  const int left = k > 0 ? c.unit[k - 1] : -1;  // (k - 1 >= base: the slice begins a unit before the first unit of a state)
  if (t == 1) st.arc[0] = AliArc{a0 + j, s0, g, left, c.unit[k], entered};
  if (t == c.T) return st;
  int a = fab[t] + (entered ? f.degsum(f.kE0, j) : f.degsum(f.kE0, f.nE) + f.degsum(f.kL0, j - f.nE));
  const AliFrame f1 = ali_frame(c.lo, c.hi, c.n, c.Tu, c.o + t + 1, f.a1, f.h0);
  const int next = fsb[t + 1];
  if (f.enters(k)) st.arc[1] = AliArc{a++, g, next + (k + 1 - f1.kE0), c.unit[k], c.unit[k + 1], true};
  if (f.stays(k)) st.arc[2] = AliArc{a, g, next + f1.nE + (k - f1.kL0), left, c.unit[k], false};
  return st;
}

inline std::string alignment_message(const char *fmt, const char *who, int a = 0, int b = 0, int c = 0, int d = 0) {
  char buf[512];
  snprintf(buf, sizeof(buf), fmt, who, a, b, c, d);
  return buf;
}

// The units of one sequence against its T frames (an utterance's, for a chunk); false with *err set.
inline bool alignment_sequence_validate(const char *who, const TranscriptUnits &u, int s, int T, int n, const int *units, const int *starts,
                                        std::string *err) {
  if (n < 1) {
    *err = alignment_message("%ssequence %d has %d units: an alignment has one at least (unit_begin must not decrease)", who, s, n);
    return false;
  }
  for (int k = 0; k < n; k++) {
    const int b = starts[k];
    if (units[k] < 0 || units[k] >= u.U) {
      *err = alignment_message("%ssequence %d unit %d: unit %d outside [0, %d)", who, s, k, units[k], u.U);
      return false;
    }
    if (k == 0 && b != 0) {
      *err = alignment_message("%ssequence %d unit 0: starts at frame %d, the first unit starts at frame 0", who, s, b);
      return false;
    }
    if (k > 0 && b <= starts[k - 1]) {
      *err = alignment_message("%ssequence %d unit %d: starts at frame %d, not behind the start %d of the unit before it", who, s, k, b, starts[k - 1]);
      return false;
    }
    if (b >= T) {
      *err = alignment_message("%ssequence %d unit %d: starts at frame %d, outside the %d frames of a sequence", who, s, k, b, T);
      return false;
    }
  }
  return true;
}

// What every entry that takes alignments refuses; false with *err set.  who: the prefix of the messages, the call's name.
// chunks: the entries that take chunks of whole-utterance alignments -- sequence s is the frames [chunk_begin[s], chunk_begin[s] + T) of an
// utterance of utt_frames[s] frames, whose alignment the units and starts are; else both arrays are null and a sequence has T frames.
inline bool alignments_validate(const char *who, const TranscriptUnits &u, int B, int T, const int *unit_begin, const int *units, const int *starts,
                                int tolerance, std::string *err, bool chunks = false, const int *utt_frames = nullptr, const int *chunk_begin = nullptr) {
  if (B <= 0 || T <= 0 || !unit_begin || !units || !starts || (chunks && (!utt_frames || !chunk_begin))) {
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
    if (chunks && n >= 1) {
      if (utt_frames[s] < 1) {
        *err = alignment_message("%ssequence %d: an utterance of %d frames: it has one at least", who, s, utt_frames[s]);
        return false;
      }
      if (chunk_begin[s] < 0) {
        *err = alignment_message("%ssequence %d: the chunk begins at frame %d, before the utterance", who, s, chunk_begin[s]);
        return false;
      }
      if ((long long)chunk_begin[s] + T > utt_frames[s]) {
        *err = alignment_message("%ssequence %d: the chunk of %d frames from frame %d ends behind the %d frames of the utterance", who, s, T, chunk_begin[s],
                                 utt_frames[s]);
        return false;
      }
    }
    if (!alignment_sequence_validate(who, u, s, chunks ? utt_frames[s] : T, n, units + k0, starts + k0, err)) return false;
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

struct AlignmentSupPlan {  // a validated minibatch as the assigns from alignments stage and record it
  SupPlan plan;
  std::vector<int> seq_state_begin, seq_arc_begin;  // [B + 1]
  std::vector<int> slice_begin;                     // [B + 1]: sequence s's staged units are [slice_begin[s], slice_begin[s + 1]) of the three below
  std::vector<int> units, lo, hi;                   // the slices, one behind the other: what the kernel reads (units: chunks only)
  std::vector<int> chunk;                           // chunks only, four ints a sequence: the utterance's frames and units, the chunk's
                                                    // first frame, the number in the utterance of the slice's first unit
};

// Plans a minibatch that alignments_validate accepted: what sup_validate and sup_widths find on the lattice's arrays, from the frames'
// closed form; and the slice of every sequence's units that the kernel needs.  utt_frames, chunk_begin, units: of chunks, else null (a
// sequence is an utterance of T frames from frame 0, its slice every unit, and the caller stages its units as they are).
// False with *err set: 2^31 states or arcs, or more.
//
// The slice of a chunk [o, o + T).  The states of the time t are the units [H(t - 1), A(t - 1)) (E) and [H(t) - 1, A(t - 2)) (L); A and H
// do not decrease, so the times o + 1 .. o + T name units of [H(o + 1) - 1, A(o + T - 1)) only (H(o) >= H(o + 1) - 1 >= 0: hi_0 = 0).  An
// arc's pdf reads its destination's unit, another state's, and that unit's left neighbour; ali_frame reads lo and hi at the counts
// themselves, the largest A(o + T - 1) (H(x) <= A(x - 1): hi_k < x needs lo_k < x).  So the slice is
//   [max(H(o + 1) - 2, 0), min(A(o + T - 1) + 1, n)).
// A unit before it has hi_k+2 <= o, so lo_k <= hi_k <= o - 2: it counts in every A(x), x >= o - 1, and H(x), x >= o.  A unit behind it
// has lo_k > lo_k-1 > o + T - 1, so hi_k >= lo_k >= o + T + 1: it counts in no A(x), x <= o + T, and no H(x), x <= o + T.  Hence the counts
// over the slice plus its base are the utterance's wherever the kernel asks (AliChunk).
inline bool alignment_chunks_plan(const char *who, int B, int T, const int *unit_begin, const int *units, const int *starts, const int *utt_frames,
                                  const int *chunk_begin, int tolerance, AlignmentSupPlan *ap, std::string *err) {
  SupPlan &p = ap->plan;
  p.max_states_per_seq = p.max_states_per_frame = p.max_arcs_per_frame = p.max_arcs_per_seq = 0;
  p.frame_state_begin.assign((size_t)B * (T + 2), 0);
  ap->seq_state_begin.assign(1, 0);
  ap->seq_arc_begin.assign(1, 0);
  ap->slice_begin.assign(1, 0);
  ap->units.clear();
  ap->lo.clear();
  ap->hi.clear();
  ap->chunk.clear();
  std::vector<int> lo, hi;  // the windows of one utterance
  long long NS = 0, NA = 0;
  for (int s = 0; s < B; s++) {
    const int k0 = unit_begin[s], n = unit_begin[s + 1] - k0;
    const int Tu = utt_frames ? utt_frames[s] : T, o = chunk_begin ? chunk_begin[s] : 0;
    lo.resize(n);
    hi.resize(n);
    alignment_windows(n, Tu, starts + k0, tolerance, lo.data(), hi.data());
    int *fsb = p.frame_state_begin.data() + (size_t)s * (T + 2);
    long long S = 1, A = 0;  // the start
    fsb[0] = (int)NS;
    p.max_states_per_frame = std::max(p.max_states_per_frame, 1);
    int a2 = (int)(std::upper_bound(lo.begin(), lo.end(), o - 1) - lo.begin());  // A(o - 1)
    int h1 = (int)(std::lower_bound(hi.begin(), hi.end(), o) - hi.begin());      // H(o)
    int first = 0, last = n;  // H(o + 1) and A(o + T - 1)
    for (int t = 1; t <= T; t++) {
      const AliFrame f = ali_frame(lo.data(), hi.data(), n, Tu, o + t, a2, h1);
      // the arcs that leave the frame before: the start's, one into every state of time 1; none leave the last frame
      const int arcs_before = t == 1 ? f.states() : 0, arcs = t < T ? f.arcs() : 0;
      A += arcs_before;
      p.max_arcs_per_frame = std::max(p.max_arcs_per_frame, arcs_before);
      if (NS + S >= (1ll << 31) || NA + A >= (1ll << 31)) break;
      fsb[t] = (int)(NS + S);
      S += f.states();
      A += arcs;
      p.max_states_per_frame = std::max(p.max_states_per_frame, f.states());
      p.max_arcs_per_frame = std::max(p.max_arcs_per_frame, arcs);
      if (t == 1) first = f.h0;
      if (t == T) last = f.a1;
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
    const int base = std::max(first - 2, 0), end = std::min(last + 1, n);
    ap->lo.insert(ap->lo.end(), lo.begin() + base, lo.begin() + end);
    ap->hi.insert(ap->hi.end(), hi.begin() + base, hi.begin() + end);
    if (units) ap->units.insert(ap->units.end(), units + k0 + base, units + k0 + end);
    ap->slice_begin.push_back((int)ap->lo.size());
    if (utt_frames) ap->chunk.insert(ap->chunk.end(), {Tu, n, o, base});
  }
  p.num_states = (int)NS;
  p.num_arcs = (int)NA;
  p.wide = (long long)p.num_states > (long long)B * 4 * (T + 1);
  return true;
}

// The plan of whole alignments: every sequence the chunk [0, T) of an utterance of T frames.
inline bool alignments_plan(const char *who, int B, int T, const int *unit_begin, const int *starts, int tolerance, AlignmentSupPlan *ap,
                            std::string *err) {
  return alignment_chunks_plan(who, B, T, unit_begin, nullptr, starts, nullptr, nullptr, tolerance, ap, err);
}

// tdnnf_alignment_supervision_sizes and tdnnf_alignment_chunk_supervision_sizes but for the handle: the states and arcs of every
// sequence's lattice (either out-pointer may be null), refusing what the assign refuses.  chunks: as alignments_validate.
inline bool alignment_sizes(const char *who, const TranscriptUnits &u, int B, int T, const int *unit_begin, const int *units, const int *starts,
                            int tolerance, int *states_out, int *arcs_out, std::string *err, bool chunks = false, const int *utt_frames = nullptr,
                            const int *chunk_begin = nullptr) {
  AlignmentSupPlan ap;
  if (!alignments_validate(who, u, B, T, unit_begin, units, starts, tolerance, err, chunks, utt_frames, chunk_begin) ||
      !alignment_chunks_plan(who, B, T, unit_begin, nullptr, starts, utt_frames, chunk_begin, tolerance, &ap, err))
    return false;
  for (int s = 0; s < B; s++) {
    if (states_out) states_out[s] = ap.seq_state_begin[s + 1] - ap.seq_state_begin[s];
    if (arcs_out) arcs_out[s] = ap.seq_arc_begin[s + 1] - ap.seq_arc_begin[s];
  }
  return true;
}

// The ints an assign of chunks stages in front of the supervision's begins and frame_state_begin (the raw prefix, which the kernel
// reads in the device staging): the arc begins, the slice begins, three ints a staged unit and four a sequence.
inline size_t alignment_chunks_raw_ints(int B, const AlignmentSupPlan &ap) { return 2 * ((size_t)B + 1) + 3 * ap.lo.size() + 4 * (size_t)B; }

// The staging's two shapes against the bytes tdnnf_supervision_reserve made (sup_stage_bytes): on the host the raw prefix, the
// supervision's begins and frame_state_begin; on the device the raw prefix and behind it the four arc arrays the kernel writes.  The
// reserve sized it for 8 bytes a state and 16 an arc, which a minibatch of short chunks may fall short of (a one-frame chunk: 2 states,
// 1 arc, up to 3 staged units).  False with *err naming the shortfall.
inline bool alignment_chunks_fit_staging(const char *who, int B, const AlignmentSupPlan &ap, size_t stage_bytes, std::string *err) {
  const size_t raw = alignment_chunks_raw_ints(B, ap);
  const size_t host = sizeof(int) * (raw + (size_t)B + 1 + ap.plan.frame_state_begin.size()), dev = sizeof(int) * (raw + 4 * (size_t)ap.plan.num_arcs);
  const size_t need = std::max(host, dev);
  if (need <= stage_bytes) return true;
  char buf[512];
  snprintf(buf, sizeof(buf),
           "%sthe chunks' %zu staged units need %zu bytes of staging, the supervision has %zu: short by %zu (reserve more states or arcs: 8 bytes a "
           "state, 16 an arc)",
           who, ap.lo.size(), need, stage_bytes, need - stage_bytes);
  *err = buf;
  return false;
}

}  // namespace tdnnf

#ifdef __HIP__  // (the compiler's own mark of a .hip file: g++ sees the plain half only)
#include "align_graphs.h"

namespace tdnnf {

// What the compile kernel (chain_sup_compile_kernels.h) takes by value; chain_sup_compile.hip launches it.
struct SupCompileDev {
  int B, T;
  int cap_states, cap_arcs;
  const int *slice_begin, *seq_arc_begin;           // [B + 1] (device staging)
  const int *units, *lo, *hi;                       // [staged units] (device staging): sequence s's are [slice_begin[s], slice_begin[s + 1])
  const int *chunk;                                 // [4 * B] (device staging) AlignmentSupPlan::chunk; null: whole alignments, every sequence
                                                    // an utterance of T frames from frame 0 with all its units staged
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
