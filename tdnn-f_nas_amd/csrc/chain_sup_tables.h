// chain_sup_tables.h -- the host side of assigning a minibatch to a reserved time-synchronous supervision (include/tdnnf_hip.h,
// tdnnf_supervision_reserve / tdnnf_supervision_assign): what tdnnf_supervision_create refuses, in its words under the caller's name, the
// four capacities, frame_state_begin (it falls out of the validation), and what launch planning needs of the minibatch -- the widths and
// `wide` -- without building an arc table: O(states + arcs + B * T).  The tables themselves are built on the device
// (chain_sup_build_kernels.h).  Plain C++ with no device header, so that a test builds it with g++ (tests/supervision_driver.cc under the
// address and undefined-behaviour sanitizers, tests/test_supervision_tables_ref.py).
#pragma once
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

#include "assign_stage.h"

namespace tdnnf {

inline std::string sup_message(const char *fmt, const char *who, int a = 0, int b = 0, int c = 0) {
  char buf[512];
  snprintf(buf, sizeof(buf), fmt, who, a, b, c);
  return buf;
}

struct SupPlan {  // a validated minibatch as tdnnf_supervision_assign stages and records it
  int num_states, num_arcs;
  int max_states_per_seq, max_states_per_frame, max_arcs_per_frame, max_arcs_per_seq;
  bool wide;                          // tdnnf_supervision_create's rule: num_states > B * 4 * (T + 1)
  std::vector<int> frame_state_begin;  // [B * (T + 2)]: [s * (T + 2) + t] = the first state of sequence s with time >= t
};

// What tdnnf_supervision_create refuses, condition for condition and in its order; false with *err set.  who: the prefix of the messages,
// the call's name.  On top of that -- tdnnf_supervision_create reads such arrays out of bounds, the device build would write so -- the two
// begin arrays must start at 0 and seq_arc_begin must not decrease.  Fills p->frame_state_begin, num_states, num_arcs, max_states_per_seq.
inline bool sup_validate(const char *who, bool have_out, int B, int T, const int *seq_state_begin, const int *seq_arc_begin, const int *state_time,
                         const float *final_logprob, const int *arc_src, const int *arc_dst, const int *arc_pdf, const float *arc_logprob, SupPlan *p,
                         std::string *err) {
  if (!(have_out && B > 0 && T > 0 && seq_state_begin && seq_arc_begin && state_time && final_logprob && arc_src && arc_dst && arc_pdf && arc_logprob)) {
    *err = sup_message("%sbad arguments", who);
    return false;
  }
  if (seq_state_begin[0] != 0 || seq_arc_begin[0] != 0) {
    *err = sup_message("%sseq_state_begin and seq_arc_begin must start at 0", who);
    return false;
  }
  for (int s = 0; s < B; s++)
    if (seq_arc_begin[s + 1] < seq_arc_begin[s]) {
      *err = sup_message("%ssequence %d has a negative arc count", who, s);
      return false;
    }
  p->num_states = seq_state_begin[B];
  p->num_arcs = seq_arc_begin[B];
  p->max_states_per_seq = p->max_arcs_per_seq = 0;
  std::vector<int> &fsb = p->frame_state_begin;
  fsb.assign((size_t)B * (T + 2), 0);
  for (int s = 0; s < B; s++) {
    const int s0 = seq_state_begin[s], s1 = seq_state_begin[s + 1];
    p->max_states_per_seq = std::max(p->max_states_per_seq, s1 - s0);
    p->max_arcs_per_seq = std::max(p->max_arcs_per_seq, seq_arc_begin[s + 1] - seq_arc_begin[s]);
    if (!(s1 > s0 && state_time[s0] == 0)) {
      *err = sup_message("%ssequence %d must start with its time-0 start state", who, s);
      return false;
    }
    int st = s0;
    for (int t = 0; t <= T + 1; t++) {
      while (st < s1 && state_time[st] < t) st++;
      fsb[(size_t)s * (T + 2) + t] = st;
    }
    for (int i = s0 + 1; i < s1; i++)
      if (!(state_time[i] >= state_time[i - 1] && state_time[i] <= T)) {
        *err = sup_message("%sstates must be sorted by time", who);
        return false;
      }
    if (fsb[(size_t)s * (T + 2) + 1] != s0 + 1) {
      *err = sup_message("%sexactly one time-0 state per sequence", who);
      return false;
    }
    for (int a = seq_arc_begin[s]; a < seq_arc_begin[s + 1]; a++)
      if (!(arc_src[a] >= s0 && arc_src[a] < s1 && arc_dst[a] >= s0 && arc_dst[a] < s1 && arc_pdf[a] >= 0 &&
            state_time[arc_dst[a]] == state_time[arc_src[a]] + 1)) {
        *err = sup_message("%sarc %d must advance exactly one frame inside its sequence", who, a);
        return false;
      }
  }
  return true;
}

// The four capacities of a reserved supervision against a validated minibatch; false with *err naming the capacity, its value and the excess.
inline bool sup_check_capacity(const char *who, int B, int T, const SupPlan &p, int max_sequences, int max_frames, int max_states, int max_arcs,
                               std::string *err) {
  return within_capacity(who, B, "sequences", max_sequences, err) && within_capacity(who, T, "frames", max_frames, err) &&
         within_capacity(who, p.num_states, "states", max_states, err) && within_capacity(who, p.num_arcs, "arcs", max_arcs, err);
}

// The widths of a minibatch that sup_validate accepted, as tdnnf_supervision_create finds them from its arc tables: the widest frame of any
// sequence, the most arcs that leave one frame (frame T included: none do), and `wide`.  An arc leaves the frame of its source state.
inline void sup_widths(int B, int T, const int *arc_src, SupPlan *p) {
  const std::vector<int> &fsb = p->frame_state_begin;
  p->wide = (long long)p->num_states > (long long)B * 4 * (T + 1);
  p->max_states_per_frame = p->max_arcs_per_frame = 0;
  std::vector<int> out_count((size_t)p->num_states + 1, 0);  // per state, then summed: out_begin without the lists
  for (int a = 0; a < p->num_arcs; a++) out_count[arc_src[a] + 1]++;
  for (int i = 0; i < p->num_states; i++) out_count[i + 1] += out_count[i];
  for (int s = 0; s < B; s++)
    for (int t = 0; t <= T; t++) {
      const int f0 = fsb[(size_t)s * (T + 2) + t], f1 = fsb[(size_t)s * (T + 2) + t + 1];
      p->max_states_per_frame = std::max(p->max_states_per_frame, f1 - f0);
      p->max_arcs_per_frame = std::max(p->max_arcs_per_frame, out_count[f1] - out_count[f0]);
    }
}

// Bytes of one staging buffer at the capacities: the two begin arrays, frame_state_begin, two arrays per state, four per arc.
inline size_t sup_stage_bytes(int max_sequences, int max_frames, int max_states, int max_arcs) {
  return sizeof(int) * (2 * ((size_t)max_sequences + 1) + (size_t)max_sequences * ((size_t)max_frames + 2) + 2 * (size_t)max_states + 4 * (size_t)max_arcs);
}

}  // namespace tdnnf
