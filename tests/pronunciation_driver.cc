// pronunciation_driver.cc -- the host side of the pronunciation compile (tdnn-f_nas_amd/csrc/align_pronunciations.h: what
// tdnnf_pronunciation_graph_sizes and tdnnf_align_graphs_assign_pronunciations run before anything reaches the device) as a stand-alone
// program, for a build under the address and undefined-behaviour sanitizers.  argv[1]: the batches of tests/pronunciation_graphs_ref.py
// with what the numpy statement finds on its arc arrays -- per batch a line "U context P G positions alternatives entries", then one line
// each: entry_pdf, loop_pdf, the six flat arrays, and the statement's state_begin, arc_begin, largest in-degrees, col_begin, col_pdfs and
// the first state of every position.  The plan made from the flat arrays alone must give exactly those; the label lists are the entries.
// Then every refusal by its message.  No device, no library.  Used by tests/test_pronunciation_plan_cpu.py.
// Build: g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I tdnn-f_nas_amd/csrc tests/pronunciation_driver.cc
#include <cstdio>
#include <cstring>
#include <limits>

#include "align_pronunciations.h"
#include "assign_stage.h"

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

static bool read_ints(FILE *f, size_t n, std::vector<int> *v) {
  v->resize(n);
  for (size_t i = 0; i < n; i++)
    if (std::fscanf(f, "%d", &(*v)[i]) != 1) return false;
  return true;
}
static bool read_floats(FILE *f, size_t n, std::vector<float> *v) {
  v->resize(n);
  for (size_t i = 0; i < n; i++)
    if (std::fscanf(f, "%f", &(*v)[i]) != 1) return false;
  return true;
}

static int plans(const char *path) {
  FILE *f = std::fopen(path, "r");
  if (!f) {
    std::printf("cannot open %s\n", path);
    return 1;
  }
  int batches = 0, U, context, P, G, NP, NQ, NE;
  while (std::fscanf(f, "%d %d %d %d %d %d %d", &U, &context, &P, &G, &NP, &NQ, &NE) == 7) {
    TranscriptUnits u;
    u.U = U;
    u.P = P;
    u.context = context;
    u.take_logprob = u.skip_logprob = 0.0f;
    const size_t n = context ? (size_t)(U + 1) * U : U;
    std::vector<int> pos_begin, pos_optional, pos_alt_begin, alt_unit_begin, alt_units, state_begin, arc_begin, in_degree, col_begin, col_pdfs, pos_state;
    std::vector<float> alt_logprob;
    bool ok = read_ints(f, n, &u.entry_pdf) && read_ints(f, n, &u.loop_pdf) && read_ints(f, G + 1, &pos_begin) && read_ints(f, NP, &pos_optional) &&
              read_ints(f, NP + 1, &pos_alt_begin) && read_floats(f, NQ, &alt_logprob) && read_ints(f, NQ + 1, &alt_unit_begin) && read_ints(f, NE, &alt_units) &&
              read_ints(f, G + 1, &state_begin) && read_ints(f, G + 1, &arc_begin) && read_ints(f, G, &in_degree) && read_ints(f, G + 1, &col_begin);
    ok = ok && read_ints(f, col_begin[G], &col_pdfs) && read_ints(f, NP, &pos_state);
    if (!ok) {
      std::printf("batch %d: short file\n", batches);
      std::fclose(f);
      return 1;
    }
    const PronunciationBatch b = {G, pos_begin.data(), pos_optional.data(), pos_alt_begin.data(), alt_logprob.data(), alt_unit_begin.data(), alt_units.data()};
    std::string err;
    EXPECT(pronunciations_validate("driver: ", u, b, &err), "batch %d: %s", batches, err.c_str());
    for (int labelled = 0; labelled < 2; labelled++) {
      PronunciationPlan p;
      EXPECT(pronunciations_plan("driver: ", u, b, labelled != 0, &p, &err), "batch %d: %s", batches, err.c_str());
      EXPECT(p.state_begin == state_begin && p.arc_begin == arc_begin, "batch %d: begins", batches);
      EXPECT(p.max_in_degree == in_degree, "batch %d: in-degrees", batches);
      EXPECT(p.col_begin == col_begin && p.col_pdfs == col_pdfs, "batch %d: pdf columns", batches);
      int max_arcs = 0, max_rows = 0, max_entries = 0;
      std::vector<int> labels, lbegin(1, 0);
      for (int g = 0; g < G; g++) {
        const int entries = alt_unit_begin[pos_alt_begin[pos_begin[g + 1]]] - alt_unit_begin[pos_alt_begin[pos_begin[g]]];
        EXPECT(p.num_arcs[g] == arc_begin[g + 1] - arc_begin[g] && p.num_cols[g] == col_begin[g + 1] - col_begin[g], "batch %d graph %d: counts", batches, g);
        EXPECT(p.num_lcols[g] == (labelled ? entries : 0), "batch %d graph %d: label columns", batches, g);
        for (int e = 0; e < entries && labelled; e++) labels.push_back(e);
        lbegin.push_back((int)labels.size());
        max_arcs = std::max(max_arcs, p.num_arcs[g]);
        max_rows = std::max(max_rows, std::max(state_begin[g + 1] - state_begin[g], std::max(p.num_cols[g], labelled ? entries : 0)));
        max_entries = std::max(max_entries, entries);
        // the sizes entry's closed form alone
        const PronunciationSize z = pronunciation_graph_size(context, pos_begin[g + 1] - pos_begin[g], pos_optional.data() + pos_begin[g],
                                                             pos_alt_begin.data() + pos_begin[g], alt_unit_begin.data());
        EXPECT(z.states == state_begin[g + 1] - state_begin[g] && z.arcs == p.num_arcs[g] && z.max_in_degree == in_degree[g] && z.entries == entries,
               "batch %d graph %d: sizes", batches, g);
      }
      EXPECT(p.col_labels == labels && p.lcol_begin == (labelled ? lbegin : std::vector<int>(1, 0)), "batch %d: label columns", batches);
      EXPECT(p.max_graph_arcs == max_arcs && p.max_graph_rows == max_rows && p.max_entries == max_entries, "batch %d: maxima", batches);
      for (int q = 0; q < NP; q++) EXPECT(p.pos_info[q] == 2 * pos_state[q] + (pos_optional[q] ? 1 : 0), "batch %d position %d: first state", batches, q);
      for (int q = 0; q < NP; q++)
        for (int a = pos_alt_begin[q]; a < pos_alt_begin[q + 1]; a++) EXPECT(p.alt_pos[a] == q, "batch %d alternative %d: position", batches, a);
      // the staging a reserve of exactly this batch's states and arcs has (align_graphs.hip), against what the device side needs
      const size_t have = 4 * ((size_t)G + 1) + 7 * (size_t)arc_begin[G] + 2 * (size_t)state_begin[G] + 2 * (size_t)G;
      EXPECT(pronunciations_raw_ints(G, NP, NQ, NE) + 4 * (size_t)arc_begin[G] <= have, "batch %d: staging", batches);
    }
    std::printf("batch: %d %d %d %d\n", G, state_begin[G], arc_begin[G], *std::max_element(in_degree.begin(), in_degree.end()));
    batches++;
  }
  std::fclose(f);
  std::printf("plans: %d batches\n", batches);
  return 0;
}

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

static void refusal(const TranscriptUnits &u, const PronunciationBatch &b, const char *want) {
  std::string err;
  const bool ok = pronunciations_validate("driver: ", u, b, &err);
  std::printf("refusal: %s\n", err.c_str());
  EXPECT(!ok && std::strstr(err.c_str(), want), "wanted '%s', got '%s'", want, err.c_str());
}

static void refusals() {
  const TranscriptUnits u = units(4, 1);
  // two transcripts: (position 0: [0 1] | [2]; position 1, optional: [3]), (position 0: [1]; position 1: [2 2] | [0] | [3]; position 2, optional: [1])
  const int pos_begin[3] = {0, 2, 5}, pos_optional[5] = {0, 1, 0, 0, 1}, pos_alt_begin[6] = {0, 2, 3, 4, 7, 8};
  const float alt_logprob[8] = {-0.5f, -1.0f, 0.0f, 0.0f, -0.25f, -0.5f, -2.0f, 0.0f};
  const int alt_unit_begin[9] = {0, 2, 3, 4, 5, 7, 8, 9, 10}, alt_units[10] = {0, 1, 2, 3, 1, 2, 2, 0, 3, 1};
  const PronunciationBatch good = {2, pos_begin, pos_optional, pos_alt_begin, alt_logprob, alt_unit_begin, alt_units};
  std::string err;
  EXPECT(pronunciations_validate("driver: ", u, good, &err), "%s", err.c_str());

  PronunciationBatch b = good;
  const int no_alternative[6] = {0, 2, 3, 4, 4, 8};  // (transcript 1 position 1 has none; position 2 takes them)
  b.pos_alt_begin = no_alternative;
  refusal(u, b, "driver: transcript 1 position 1 has 0 alternatives: a position has one at least");
  b = good;
  const int empty_alternative[9] = {0, 2, 3, 4, 5, 7, 7, 9, 10};
  b.alt_unit_begin = empty_alternative;
  refusal(u, b, "driver: transcript 1 position 1 alternative 1 has 0 units: an alternative has one at least");
  b = good;
  const int bad_units[10] = {0, 1, 2, 3, 1, 2, 4, 0, 3, 1};
  b.alt_units = bad_units;
  refusal(u, b, "driver: transcript 1 position 1 alternative 0: unit 4 (its number 1) outside [0, 4)");
  const int negative_units[10] = {0, 1, -1, 3, 1, 2, 2, 0, 3, 1};
  b.alt_units = negative_units;
  refusal(u, b, "driver: transcript 0 position 0 alternative 1: unit -1 (its number 0) outside [0, 4)");
  b = good;
  float nan_logprob[8], inf_logprob[8];
  std::memcpy(nan_logprob, alt_logprob, sizeof(nan_logprob));
  std::memcpy(inf_logprob, alt_logprob, sizeof(inf_logprob));
  nan_logprob[6] = std::numeric_limits<float>::quiet_NaN();
  inf_logprob[1] = -std::numeric_limits<float>::infinity();
  b.alt_logprob = nan_logprob;
  refusal(u, b, "driver: transcript 1 position 1 alternative 2: alt_logprob is NaN or infinite");
  b.alt_logprob = inf_logprob;
  refusal(u, b, "driver: transcript 0 position 0 alternative 1: alt_logprob is NaN or infinite");
  b = good;
  const int adjacent[5] = {0, 1, 0, 1, 1};
  b.pos_optional = adjacent;
  refusal(u, b, "driver: transcript 1 position 2: optional, as is position 1 before it (adjacent optional positions are not supported)");
  b = good;
  const int one_begin[3] = {0, 2, 3}, all_optional[3] = {0, 1, 1};  // (transcript 1 is its one position)
  b.pos_begin = one_begin;
  b.pos_optional = all_optional;
  refusal(u, b, "driver: transcript 1 position 0: optional, and the transcript has no mandatory position");
  b = good;
  const int empty_begin[3] = {0, 0, 5};
  b.pos_begin = empty_begin;
  refusal(u, b, "driver: transcript 0 has 0 positions: a transcript has one at least");
  b = good;
  b.G = 0;
  refusal(u, b, "driver: bad arguments (num_transcripts 0, or a null array)");
  b = good;
  b.alt_logprob = nullptr;
  refusal(u, b, "driver: bad arguments (num_transcripts 2, or a null array)");
  b = good;
  const int late_begin[9] = {1, 2, 3, 4, 5, 7, 8, 9, 10};
  b.alt_unit_begin = late_begin;
  refusal(u, b, "driver: pos_begin, pos_alt_begin and alt_unit_begin must start at 0");

  // the capacities and num_labels, in assign's words (assign_stage.h: what align_graphs.hip says with these numbers)
  PronunciationPlan p;
  EXPECT(pronunciations_plan("driver: ", u, good, true, &p, &err), "%s", err.c_str());
  const int NS = p.state_begin[2], NA = p.arc_begin[2];
  const char *what[3] = {"graphs", "states", "arcs"};
  const int n[3] = {2, NS, NA};
  for (int i = 0; i < 3; i++) {
    EXPECT(within_capacity("driver: ", n[i], what[i], n[i], &err), "%s at its capacity", what[i]);
    EXPECT(!within_capacity("driver: ", n[i], what[i], n[i] - 1, &err), "%s one over", what[i]);
    std::printf("capacity: %s\n", err.c_str());
    char want[128];
    std::snprintf(want, sizeof(want), "driver: %d %s exceed the capacity max_%s = %d by 1", n[i], what[i], what[i], n[i] - 1);
    EXPECT(err == want, "wanted '%s', got '%s'", want, err.c_str());
  }
  EXPECT(p.max_entries == 6, "%d", p.max_entries);
}

int main(int argc, char **argv) {
  if (argc != 2) {
    std::printf("usage: pronunciation_driver <batches file>\n");
    return 2;
  }
  if (int rc = plans(argv[1])) return rc;
  refusals();
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
