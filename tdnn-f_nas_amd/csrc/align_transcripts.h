// align_transcripts.h -- the host side of compiling transcript graphs (include/tdnnf_hip.h, "transcript graphs"): what a unit set keeps on
// the host, the validation of a batch of transcripts, and everything tdnnf_align_graphs_assign_transcripts needs to know of the graphs
// without ever holding an arc -- the states and arcs of every graph from the closed forms, its largest in-degree, its column lists.  O(slots)
// apart from the sort of a graph's pdfs.  Plain C++ with no device header, so that a test builds it with g++ (tests/transcript_driver.cc
// under the address and undefined-behaviour sanitizers, tests/test_transcript_graphs_ref.py); the kernel that writes the arcs is
// align_compile_kernels.h.
//
// The graph of a transcript of n slots (unit u_k, optional flag opt_k): state 0 is the start; for every slot k in order state A_k (left
// neighbour slot k-1) and, only in context 1 behind an optional slot k-1, state B_k (left neighbour slot k-2: slot k-1 was skipped).  Every
// state of slot k has a self-loop, an arc into A_k+1 and, over an optional slot k+1, an arc into B_k+2 (context 1) or A_k+2 (context 0).
#pragma once
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

namespace tdnnf {

struct TranscriptUnits {  // a unit set's tables on the host
  int U, P, context;      // units, pdfs, 0 context-independent / 1 left-biphone
  std::vector<int> entry_pdf, loop_pdf;  // context 0: [U]; context 1: [(U + 1) * U] at (left + 1) * U + u, left = -1: nothing before it
  std::vector<float> loop_logprob, leave_logprob;  // [U]
  float take_logprob, skip_logprob;
};

inline int transcript_pdf_index(const TranscriptUnits &u, int left, int unit) { return u.context ? (left + 1) * u.U + unit : unit; }

inline std::string transcript_message(const char *fmt, const char *who, int a = 0, int b = 0, int c = 0, int d = 0) {
  char buf[512];
  snprintf(buf, sizeof(buf), fmt, who, a, b, c, d);
  return buf;
}

// What every entry that takes transcripts refuses; false with *err set.  who: the prefix of the messages, the call's name.
inline bool transcripts_validate(const char *who, const TranscriptUnits &u, int num_transcripts, const int *slot_begin, const int *slot_unit,
                                 const int *slot_optional, std::string *err) {
  if (num_transcripts <= 0 || !slot_begin || !slot_unit || !slot_optional) {
    *err = transcript_message("%sbad arguments (num_transcripts %d, or a null array)", who, num_transcripts);
    return false;
  }
  if (slot_begin[0] != 0) {
    *err = transcript_message("%sslot_begin must start at 0", who);
    return false;
  }
  for (int g = 0; g < num_transcripts; g++) {
    const int k0 = slot_begin[g], n = slot_begin[g + 1] - k0;
    if (n < 1) {
      *err = transcript_message("%stranscript %d has %d slots: a transcript has one at least", who, g, n);
      return false;
    }
    bool mandatory = false;
    for (int k = 0; k < n; k++) {
      if (slot_unit[k0 + k] < 0 || slot_unit[k0 + k] >= u.U) {
        *err = transcript_message("%stranscript %d slot %d: unit %d outside [0, %d)", who, g, k, slot_unit[k0 + k], u.U);
        return false;
      }
      if (k > 0 && slot_optional[k0 + k] && slot_optional[k0 + k - 1]) {
        *err = transcript_message("%stranscript %d slot %d: optional, as is slot %d before it (adjacent optional slots are not supported)", who, g, k, k - 1);
        return false;
      }
      mandatory = mandatory || !slot_optional[k0 + k];
    }
    if (!mandatory) {  // (behind the check above: a transcript of the one slot)
      *err = transcript_message("%stranscript %d slot %d: optional, and the transcript has no mandatory slot", who, g, n - 1);
      return false;
    }
  }
  return true;
}

// The states and arcs of one validated transcript: S = 1 + n + #B; every state of slot k has 1 + [k+1 < n] + [k+2 < n and opt_k+1] arcs,
// the start 1 + [n >= 2 and opt_0].  *max_in_degree (optional): the largest number of arcs into one state, at most 3.
inline void transcript_graph_size(int context, int n, const int *opt, int *states, int *arcs, int *max_in_degree = nullptr) {
  int S = 1, A = 1 + (n >= 2 && opt[0] ? 1 : 0), deg = 0;
  int count_m1 = 1, count_m2 = 1;  // the states of slots k-1 and k-2; the start stands in for a slot before the first
  for (int k = 0; k < n; k++) {
    const bool behind_optional = k >= 1 && opt[k - 1];
    const int count = 1 + (context && behind_optional ? 1 : 0);
    const int out = 1 + (k + 1 < n ? 1 : 0) + (k + 2 < n && opt[k + 1] ? 1 : 0);
    S += count;
    A += count * out;
    // into A_k: its loop, the states of slot k-1 and, in context 0, over an optional slot k-1 the states of slot k-2; into B_k: its loop and
    // the states of slot k-2
    deg = std::max(deg, 1 + count_m1 + (!context && behind_optional ? count_m2 : 0));
    if (count == 2) deg = std::max(deg, 1 + count_m2);
    count_m2 = count_m1;
    count_m1 = count;
  }
  *states = S;
  *arcs = A;
  if (max_in_degree) *max_in_degree = deg;
}

// One graph's column list from `list` (its arcs' pdfs or labels, any order): the ascending distinct values behind cols, the new end behind
// begin; their number.
inline int append_columns(std::vector<int> *list, std::vector<int> *begin, std::vector<int> *cols) {
  std::sort(list->begin(), list->end());
  list->erase(std::unique(list->begin(), list->end()), list->end());
  cols->insert(cols->end(), list->begin(), list->end());
  begin->push_back((int)cols->size());
  return (int)list->size();
}

struct TranscriptPlan {  // a validated batch as tdnnf_align_graphs_assign_transcripts stages and records it
  std::vector<int> state_begin, arc_begin;             // [G + 1]
  std::vector<int> num_arcs, max_in_degree;            // [G]
  std::vector<int> col_begin, col_pdfs, num_cols;      // the ascending distinct pdfs of every graph
  std::vector<int> lcol_begin, col_labels, num_lcols;  // labelled: the labels of every graph, its slots 0 .. n-1
  std::vector<int> packed;                             // per slot 2 * unit + optional: what the kernel reads
  int max_graph_arcs, max_graph_rows, max_slots;
};

// Plans a batch that transcripts_validate accepted.  False with *err set: more than 2^31 - 1 states or arcs.
inline bool transcripts_plan(const char *who, const TranscriptUnits &u, int G, const int *slot_begin, const int *slot_unit, const int *slot_optional,
                             bool labelled, TranscriptPlan *p, std::string *err) {
  *p = TranscriptPlan();
  p->state_begin.assign(1, 0);
  p->arc_begin.assign(1, 0);
  p->col_begin.assign(1, 0);
  p->lcol_begin.assign(1, 0);
  p->max_graph_arcs = p->max_graph_rows = p->max_slots = 0;
  p->packed.resize(slot_begin[G]);
  std::vector<int> list;
  long long NS = 0, NA = 0;
  for (int g = 0; g < G; g++) {
    const int k0 = slot_begin[g], n = slot_begin[g + 1] - k0;
    const int *unit = slot_unit + k0, *opt = slot_optional + k0;
    int S, A, deg;
    transcript_graph_size(u.context, n, opt, &S, &A, &deg);
    NS += S;
    NA += A;
    if (NS >= (1ll << 31) || NA >= (1ll << 31)) {
      *err = transcript_message("%sthe batch has more than 2^31 states or arcs (at transcript %d)", who, g);
      return false;
    }
    p->state_begin.push_back((int)NS);
    p->arc_begin.push_back((int)NA);
    p->num_arcs.push_back(A);
    p->max_in_degree.push_back(deg);
    // every state has its loop and an arc into it: the graph's pdfs are its states' two
    list.clear();
    for (int k = 0; k < n; k++) {
      p->packed[k0 + k] = 2 * unit[k] + (opt[k] ? 1 : 0);
      const int a = transcript_pdf_index(u, k >= 1 ? unit[k - 1] : -1, unit[k]);
      list.push_back(u.entry_pdf[a]);
      list.push_back(u.loop_pdf[a]);
      if (u.context && k >= 1 && opt[k - 1]) {
        const int b = transcript_pdf_index(u, k >= 2 ? unit[k - 2] : -1, unit[k]);
        list.push_back(u.entry_pdf[b]);
        list.push_back(u.loop_pdf[b]);
      }
    }
    p->num_cols.push_back(append_columns(&list, &p->col_begin, &p->col_pdfs));
    int rows = std::max(S, (int)list.size());
    if (labelled) {  // an arc's label is the slot of its destination, and every slot has a state
      for (int k = 0; k < n; k++) p->col_labels.push_back(k);
      p->lcol_begin.push_back((int)p->col_labels.size());
      p->num_lcols.push_back(n);
      rows = std::max(rows, n);
    }
    p->max_graph_arcs = std::max(p->max_graph_arcs, A);
    p->max_graph_rows = std::max(p->max_graph_rows, rows);
    p->max_slots = std::max(p->max_slots, n);
  }
  if (!labelled) p->num_lcols.assign(G, 0);
  return true;
}

}  // namespace tdnnf
