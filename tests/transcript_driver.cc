// transcript_driver.cc -- the host side of the transcript compile (tdnn-f_nas_amd/csrc/align_transcripts.h: what tdnnf_transcript_graph_sizes
// and tdnnf_align_graphs_assign_transcripts run before anything reaches the device) as a stand-alone program, for a build under the address
// and undefined-behaviour sanitizers.  It validates good and refused batches, and for EVERY pattern of optional slots of up to 11 slots, in
// both contexts, holds the closed forms and the plan against a graph it builds arc by arc from the definition.  No device, no library.
// Used by tests/test_transcript_adapter_compile.py.
// Build: g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I tdnn-f_nas_amd/csrc tests/transcript_driver.cc
#include <cstdio>
#include <cstring>
#include <set>
#include <utility>

#include "align_transcripts.h"

using namespace tdnnf;

static int failures = 0;
#define EXPECT(cond, ...)          \
  do {                             \
    if (!(cond)) {                 \
      std::printf("FAILED %s: ", #cond); \
      std::printf(__VA_ARGS__);    \
      std::printf("\n");           \
      failures++;                  \
    }                              \
  } while (0)

static TranscriptUnits units(int U, int context) {
  TranscriptUnits u;
  u.U = U;
  u.context = context;
  const int n = context ? (U + 1) * U : U;
  u.P = 2 * n;
  for (int i = 0; i < n; i++) {
    u.entry_pdf.push_back((7 * i + 3) % u.P);
    u.loop_pdf.push_back((5 * i + 1) % u.P);
  }
  u.loop_logprob.assign(U, -0.5f);
  u.leave_logprob.assign(U, -1.0f);
  u.take_logprob = -0.25f;
  u.skip_logprob = -2.0f;
  return u;
}

// the definition, arc by arc: the states, the arcs as (source, destination) pairs, the pdfs they carry and the in-degrees
struct Naive {
  int S;
  std::set<std::pair<int, int>> arcs;
  std::set<int> pdfs;
  int max_in_degree;
};
static Naive naive(const TranscriptUnits &u, int n, const int *unit, const int *opt) {
  std::vector<std::vector<int>> of_slot(n);
  std::vector<int> left(1, -1), slot(1, -1);  // per state: the unit of its left neighbour, its slot
  for (int k = 0; k < n; k++) {
    of_slot[k].push_back((int)left.size());
    left.push_back(k >= 1 ? unit[k - 1] : -1);
    slot.push_back(k);
    if (u.context && k >= 1 && opt[k - 1]) {
      of_slot[k].push_back((int)left.size());
      left.push_back(k >= 2 ? unit[k - 2] : -1);
      slot.push_back(k);
    }
  }
  Naive g;
  g.S = (int)left.size();
  std::vector<int> in(g.S, 0);
  const auto add = [&](int src, int dst, bool loop) {
    const int i = transcript_pdf_index(u, left[dst], unit[slot[dst]]);
    g.pdfs.insert(loop ? u.loop_pdf[i] : u.entry_pdf[i]);
    if (g.arcs.insert({src, dst}).second) in[dst]++;
  };
  const std::vector<int> start(1, 0);
  for (int k = 0; k < n; k++) {
    for (int s : of_slot[k]) add(s, s, true);
    for (int s : k ? of_slot[k - 1] : start) add(s, of_slot[k][0], false);
    if (k >= 1 && opt[k - 1])
      for (int s : k >= 2 ? of_slot[k - 2] : start) add(s, u.context ? of_slot[k][1] : of_slot[k][0], false);
  }
  g.max_in_degree = *std::max_element(in.begin(), in.end());
  return g;
}

static void sizes_and_plans() {
  int cases = 0;
  for (int context = 0; context < 2; context++) {
    const TranscriptUnits u = units(4, context);
    for (int n = 1; n <= 11; n++)
      for (unsigned mask = 0; mask < 1u << n; mask++) {
        if ((mask & (mask >> 1)) || mask == (1u << n) - 1) continue;  // adjacent optional slots, or no mandatory slot
        std::vector<int> unit(n), opt(n);
        for (int k = 0; k < n; k++) {
          unit[k] = (3 * k + (int)mask) % u.U;
          opt[k] = (mask >> k) & 1;
        }
        const int begin[2] = {0, n};
        std::string err;
        EXPECT(transcripts_validate("driver: ", u, 1, begin, unit.data(), opt.data(), &err), "n %d mask %u: %s", n, mask, err.c_str());
        const Naive g = naive(u, n, unit.data(), opt.data());
        int S, A, deg;
        transcript_graph_size(context, n, opt.data(), &S, &A, &deg);
        EXPECT(S == g.S && A == (int)g.arcs.size() && deg == g.max_in_degree && deg <= 3, "context %d n %d mask %u: %d %d %d against %d %zu %d", context, n,
               mask, S, A, deg, g.S, g.arcs.size(), g.max_in_degree);
        TranscriptPlan p;
        EXPECT(transcripts_plan("driver: ", u, 1, begin, unit.data(), opt.data(), true, &p, &err), "%s", err.c_str());
        EXPECT(p.state_begin.back() == g.S && p.arc_begin.back() == A && p.num_arcs[0] == A && p.max_in_degree[0] == deg, "plan n %d mask %u", n, mask);
        EXPECT(p.col_pdfs == std::vector<int>(g.pdfs.begin(), g.pdfs.end()) && p.num_cols[0] == (int)g.pdfs.size(), "columns n %d mask %u", n, mask);
        EXPECT((int)p.col_labels.size() == n && p.col_labels.back() == n - 1 && p.max_slots == n && (int)p.packed.size() == n, "labels n %d mask %u", n, mask);
        cases++;
      }
  }
  std::printf("sizes and plans: %d transcripts\n", cases);
  EXPECT(cases > 400, "%d", cases);
}

static void refusal(const TranscriptUnits &u, int G, const int *begin, const int *unit, const int *opt, const char *want) {
  std::string err;
  const bool ok = transcripts_validate("driver: ", u, G, begin, unit, opt, &err);
  std::printf("refusal: %s\n", err.c_str());
  EXPECT(!ok && std::strstr(err.c_str(), want), "wanted '%s', got '%s'", want, err.c_str());
}

static void refusals() {
  const TranscriptUnits u = units(4, 1);
  const int begin[3] = {0, 2, 6};
  const int good_unit[6] = {0, 1, 2, 3, 0, 1}, good_opt[6] = {1, 0, 0, 1, 0, 1};
  std::string err;
  EXPECT(transcripts_validate("driver: ", u, 2, begin, good_unit, good_opt, &err), "%s", err.c_str());
  const int bad_unit[6] = {0, 1, 2, 3, 4, 1};
  refusal(u, 2, begin, bad_unit, good_opt, "driver: transcript 1 slot 2: unit 4 outside [0, 4)");
  const int adjacent[6] = {1, 0, 0, 0, 1, 1};
  refusal(u, 2, begin, good_unit, adjacent, "driver: transcript 1 slot 3: optional, as is slot 2 before it");
  const int one_begin[3] = {0, 2, 3}, all_optional[3] = {0, 0, 1};
  refusal(u, 2, one_begin, good_unit, all_optional, "driver: transcript 1 slot 0: optional, and the transcript has no mandatory slot");
  const int empty_begin[3] = {0, 0, 3};
  refusal(u, 2, empty_begin, good_unit, good_opt, "driver: transcript 0 has 0 slots");
  refusal(u, 0, begin, good_unit, good_opt, "driver: bad arguments");
  refusal(u, 2, nullptr, good_unit, good_opt, "driver: bad arguments");
  const int late_begin[3] = {1, 2, 6};
  refusal(u, 2, late_begin, good_unit, good_opt, "driver: slot_begin must start at 0");
}

int main() {
  sizes_and_plans();
  refusals();
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
