// align_pronunciations.h -- the host side of compiling transcripts with pronunciation alternatives (include/tdnnf_hip.h, "PRONUNCIATION
// GRAPHS"): the validation of a batch, and everything tdnnf_align_graphs_assign_pronunciations needs to know of the graphs without ever
// holding an arc -- the states and arcs of every graph from closed forms, its largest in-degree, its column lists, and the per-position and
// per-alternative tables the kernel reads.  O(entries + first-entry states) apart from the sort of a graph's pdfs.  Plain C++ with no device
// header, so that a test builds it with g++ (tests/pronunciation_driver.cc under the address and undefined-behaviour sanitizers); the kernel
// that writes the arcs is align_pron_compile_kernels.h.
//
// The graph of a transcript of n positions (flag opt_p, A_p alternatives of L units each): state 0 is the start; the entries -- one unit of
// one alternative -- follow in flat order (position, alternative, unit).  An inner entry has one state.  A first entry has one state in
// context 0 and N_p in context 1, one per predecessor: the alternatives of position p-1 (the start for p = 0) and, behind an optional
// position p-1, those of position p-2 (the start for p = 1).  Every state of an entry has a self-loop and either the arc to the next entry
// of its alternative or, from a last entry, F_p = A_p+1 + [opt_p+1] A_p+2 arcs into the first entries that it precedes.
#pragma once
#include <math.h>

#include "align_transcripts.h"

namespace tdnnf {

struct PronunciationBatch {  // the flat arrays of a batch as the C entries take them
  int G;                     // transcripts
  const int *pos_begin;      // [G + 1] a transcript's positions
  const int *pos_optional;   // [positions]
  const int *pos_alt_begin;  // [positions + 1] a position's alternatives
  const float *alt_logprob;  // [alternatives]
  const int *alt_unit_begin; // [alternatives + 1] an alternative's units: the entries
  const int *alt_units;      // [entries]
};

// What every entry that takes pronunciation transcripts refuses; false with *err set.  who: the prefix of the messages, the call's name.
inline bool pronunciations_validate(const char *who, const TranscriptUnits &u, const PronunciationBatch &b, std::string *err) {
  if (b.G <= 0 || !b.pos_begin || !b.pos_optional || !b.pos_alt_begin || !b.alt_logprob || !b.alt_unit_begin || !b.alt_units) {
    *err = transcript_message("%sbad arguments (num_transcripts %d, or a null array)", who, b.G);
    return false;
  }
  if (b.pos_begin[0] != 0 || b.pos_alt_begin[0] != 0 || b.alt_unit_begin[0] != 0) {
    *err = transcript_message("%spos_begin, pos_alt_begin and alt_unit_begin must start at 0", who);
    return false;
  }
  for (int g = 0; g < b.G; g++) {
    const int p0 = b.pos_begin[g], n = b.pos_begin[g + 1] - p0;
    if (n < 1) {
      *err = transcript_message("%stranscript %d has %d positions: a transcript has one at least", who, g, n);
      return false;
    }
    bool mandatory = false;
    for (int p = 0; p < n; p++) {
      const int q0 = b.pos_alt_begin[p0 + p], A = b.pos_alt_begin[p0 + p + 1] - q0;
      if (A < 1) {
        *err = transcript_message("%stranscript %d position %d has %d alternatives: a position has one at least", who, g, p, A);
        return false;
      }
      for (int a = 0; a < A; a++) {
        const int e0 = b.alt_unit_begin[q0 + a], L = b.alt_unit_begin[q0 + a + 1] - e0;
        if (L < 1) {
          *err = transcript_message("%stranscript %d position %d alternative %d has %d units: an alternative has one at least", who, g, p, a, L);
          return false;
        }
        for (int j = 0; j < L; j++)
          if (b.alt_units[e0 + j] < 0 || b.alt_units[e0 + j] >= u.U) {
            char buf[512];
            snprintf(buf, sizeof(buf), "%stranscript %d position %d alternative %d: unit %d (its number %d) outside [0, %d)", who, g, p, a, b.alt_units[e0 + j], j,
                     u.U);
            *err = buf;
            return false;
          }
        if (!isfinite(b.alt_logprob[q0 + a])) {
          *err = transcript_message("%stranscript %d position %d alternative %d: alt_logprob is NaN or infinite", who, g, p, a);
          return false;
        }
      }
      if (p > 0 && b.pos_optional[p0 + p] && b.pos_optional[p0 + p - 1]) {
        *err = transcript_message("%stranscript %d position %d: optional, as is position %d before it (adjacent optional positions are not supported)", who, g,
                                  p, p - 1);
        return false;
      }
      mandatory = mandatory || !b.pos_optional[p0 + p];
    }
    if (!mandatory) {  // (behind the check above: a transcript of the one position)
      *err = transcript_message("%stranscript %d position %d: optional, and the transcript has no mandatory position", who, g, n - 1);
      return false;
    }
  }
  return true;
}

struct PronunciationSize {  // one validated transcript's graph
  long long states, arcs;
  int max_in_degree, entries;
};

// The states and arcs of one validated transcript from the closed forms.  opt, alt_begin: the transcript's share of pos_optional and
// pos_alt_begin (n and n + 1 entries); alt_unit_begin: the batch's.  pos_state (optional, n entries): the first state of every position,
// local to the graph.
//   states: 1 + sum over the alternatives of N_p + L - 1                       (context 0: N_p = 1)
//   arcs:   F_-1 + sum over the alternatives of  N_p (1 + F_p)                    for L = 1
//                                                2 N_p + 2 (L - 2) + (1 + F_p)    for L >= 2
//   in-degree: a first entry's state in context 1 has its loop and the states of its predecessor's last entry -- N_q of them where that
//   alternative has one unit, else one; in context 0 its loop and every predecessor's one state.  The second entry of an alternative has
//   1 + N_p, every later one 2.
inline PronunciationSize pronunciation_graph_size(int context, int n, const int *opt, const int *alt_begin, const int *alt_unit_begin, int *pos_state = nullptr) {
  const auto alts = [&](int p) { return p < 0 ? 1 : alt_begin[p + 1] - alt_begin[p]; };  // (the start stands in for a position -1)
  const auto fan = [&](int p) { return (p + 1 < n ? alts(p + 1) : 0) + (p + 2 < n && opt[p + 1] ? alts(p + 2) : 0); };
  PronunciationSize z = {1, fan(-1), 0, alt_unit_begin[alt_begin[n]] - alt_unit_begin[alt_begin[0]]};
  int last_m1 = 1, last_m2 = 1;  // the most states of a last entry of positions p-1 and p-2; the start's one
  for (int p = 0; p < n; p++) {
    const bool behind_optional = p >= 1 && opt[p - 1];
    const int preds = alts(p - 1) + (behind_optional ? alts(p - 2) : 0);
    const int N = context ? preds : 1, F = fan(p);
    if (pos_state) pos_state[p] = (int)std::min<long long>(z.states, 0x7fffffff);
    z.max_in_degree = std::max(z.max_in_degree, context ? 1 + std::max(last_m1, behind_optional ? last_m2 : 0) : 1 + preds);
    int last = 1;
    for (int q = alt_begin[p]; q < alt_begin[p + 1]; q++) {
      const int L = alt_unit_begin[q + 1] - alt_unit_begin[q];
      z.states += N + L - 1;
      z.arcs += L == 1 ? (long long)N * (1 + F) : 2ll * N + 2ll * (L - 2) + 1 + F;
      if (L >= 2) z.max_in_degree = std::max(z.max_in_degree, 1 + N);
      if (L == 1) last = N;
    }
    last_m2 = last_m1;
    last_m1 = last;
  }
  return z;
}

struct PronunciationPlan : TranscriptPlan {  // a validated batch as tdnnf_align_graphs_assign_pronunciations stages and records it; `packed` and
                                             // `max_slots` stay empty
  std::vector<int> pos_info;                 // per position 2 * (its first state, local to its graph) + optional: what the kernel reads
  std::vector<int> alt_pos;                  // per alternative its position, as an index into the batch's positions
  int max_entries;
};

// Plans a batch that pronunciations_validate accepted.  False with *err set: more than 2^31 - 1 states or arcs.
inline bool pronunciations_plan(const char *who, const TranscriptUnits &u, const PronunciationBatch &b, bool labelled, PronunciationPlan *p, std::string *err) {
  *p = PronunciationPlan();
  p->state_begin.assign(1, 0);
  p->arc_begin.assign(1, 0);
  p->col_begin.assign(1, 0);
  p->lcol_begin.assign(1, 0);
  p->max_graph_arcs = p->max_graph_rows = p->max_slots = p->max_entries = 0;
  p->pos_info.resize(b.pos_begin[b.G]);
  p->alt_pos.resize(b.pos_alt_begin[b.pos_begin[b.G]]);
  std::vector<int> list;
  long long NS = 0, NA = 0;
  for (int g = 0; g < b.G; g++) {
    const int p0 = b.pos_begin[g], n = b.pos_begin[g + 1] - p0;
    const int *opt = b.pos_optional + p0, *alt_begin = b.pos_alt_begin + p0;
    const PronunciationSize z = pronunciation_graph_size(u.context, n, opt, alt_begin, b.alt_unit_begin, p->pos_info.data() + p0);
    NS += z.states;
    NA += z.arcs;
    if (NS >= (1ll << 31) || NA >= (1ll << 31)) {
      *err = transcript_message("%sthe batch has more than 2^31 states or arcs (at transcript %d)", who, g);
      return false;
    }
    p->state_begin.push_back((int)NS);
    p->arc_begin.push_back((int)NA);
    p->num_arcs.push_back((int)z.arcs);
    p->max_in_degree.push_back(z.max_in_degree);
    // every state has its loop and an arc into it: the graph's pdfs are its states' two
    list.clear();
    const auto state_pdfs = [&](int left, int unit) {
      const int i = transcript_pdf_index(u, left, unit);
      list.push_back(u.entry_pdf[i]);
      list.push_back(u.loop_pdf[i]);
    };
    const auto last_units = [&](int pos, int unit) {  // a first entry's states for the alternatives of position pos (the start: -1)
      if (pos < 0) return state_pdfs(-1, unit);
      for (int q = alt_begin[pos]; q < alt_begin[pos + 1]; q++) state_pdfs(b.alt_units[b.alt_unit_begin[q + 1] - 1], unit);
    };
    for (int k = 0; k < n; k++) {
      p->pos_info[p0 + k] = 2 * p->pos_info[p0 + k] + (opt[k] ? 1 : 0);
      for (int q = alt_begin[k]; q < alt_begin[k + 1]; q++) {
        p->alt_pos[q] = p0 + k;
        const int *units = b.alt_units + b.alt_unit_begin[q], L = b.alt_unit_begin[q + 1] - b.alt_unit_begin[q];
        if (u.context) {
          last_units(k - 1, units[0]);
          if (k >= 1 && opt[k - 1]) last_units(k - 2, units[0]);
        } else {
          state_pdfs(-1, units[0]);
        }
        for (int j = 1; j < L; j++) state_pdfs(units[j - 1], units[j]);
      }
    }
    p->num_cols.push_back(append_columns(&list, &p->col_begin, &p->col_pdfs));
    int rows = std::max((int)z.states, (int)list.size());
    if (labelled) {  // an arc's label is the entry of its destination, and every entry has a state
      for (int k = 0; k < z.entries; k++) p->col_labels.push_back(k);
      p->lcol_begin.push_back((int)p->col_labels.size());
      p->num_lcols.push_back(z.entries);
      rows = std::max(rows, z.entries);
    }
    p->max_graph_arcs = std::max(p->max_graph_arcs, (int)z.arcs);
    p->max_graph_rows = std::max(p->max_graph_rows, rows);
    p->max_entries = std::max(p->max_entries, z.entries);
  }
  if (!labelled) p->num_lcols.assign(b.G, 0);
  return true;
}

// The 4-byte elements a batch stages for the device in front of the arc arrays the kernel writes: five begin arrays of the graphs, the
// positions' two tables, the alternatives' three, the entries' units.
inline size_t pronunciations_raw_ints(int G, int positions, int alternatives, int entries) {
  return 5 * ((size_t)G + 1) + (2 * (size_t)positions + 1) + (3 * (size_t)alternatives + 1) + (size_t)entries;
}

}  // namespace tdnnf
