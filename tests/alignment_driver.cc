// alignment_driver.cc -- the host side of tdnnf_supervision_assign_alignments (tdnn-f_nas_amd/csrc/chain_sup_alignment.h: what runs before
// anything reaches the device) as a stand-alone program, for a build under the address and undefined-behaviour sanitizers.  Given a file of
// minibatches -- the alignments and, from the numpy statement of the lattice (tests/alignment_supervision_ref.py), the lattice's arrays;
// tests/test_alignment_plan_cpu.py writes it -- it plans each from the alignments and holds every field of the plan, both begin arrays and
// the sizes entry's answers against what sup_validate and sup_widths (chain_sup_tables.h) find on the arrays.  Then every refusal by its
// message, and the capacities one short.  No device, no library.
// Build: g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I tdnn-f_nas_amd/csrc tests/alignment_driver.cc
#include <cstdio>
#include <cstring>

#include "chain_sup_alignment.h"

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

static TranscriptUnits unit_set(int U) {
  TranscriptUnits u;
  u.U = U;
  u.P = 2 * U;
  u.context = 0;
  u.take_logprob = u.skip_logprob = 0.f;
  return u;
}

struct Alignments {
  int B, T, tol;
  std::vector<int> begin, units, starts;
};

// file: per minibatch "U B T tolerance N NS NA", then unit_begin, units, starts, and of the lattice seq_state_begin, seq_arc_begin, state_time,
// final_logprob, arc_src, arc_dst, arc_pdf, arc_logprob
static void from_file(const char *path) {
  FILE *f = std::fopen(path, "r");
  if (!f) {
    std::printf("FAILED to open %s\n", path);
    failures++;
    return;
  }
  Alignments a;
  int U, N, NS, NA, cases = 0;
  while (std::fscanf(f, "%d %d %d %d %d %d %d", &U, &a.B, &a.T, &a.tol, &N, &NS, &NA) == 7) {
    const auto ints = [&](std::vector<int> *v, int n) {
      v->assign(n, 0);
      for (int &x : *v)
        if (std::fscanf(f, "%d", &x) != 1) failures++;
    };
    const auto floats = [&](std::vector<float> *v, int n) {
      v->assign(n, 0.f);
      for (float &x : *v)
        if (std::fscanf(f, "%f", &x) != 1) failures++;
    };
    std::vector<int> ssb, sab, time, src, dst, pdf;
    std::vector<float> fin, lp;
    ints(&a.begin, a.B + 1);
    ints(&a.units, N);
    ints(&a.starts, N);
    ints(&ssb, a.B + 1);
    ints(&sab, a.B + 1);
    ints(&time, NS);
    floats(&fin, NS);
    ints(&src, NA);
    ints(&dst, NA);
    ints(&pdf, NA);
    floats(&lp, NA);
    const int B = a.B, T = a.T;
    const TranscriptUnits u = unit_set(U);
    std::string err;
    SupPlan want;
    EXPECT(sup_validate("driver: ", true, B, T, ssb.data(), sab.data(), time.data(), fin.data(), src.data(), dst.data(), pdf.data(), lp.data(), &want, &err),
           "case %d: the statement's arrays: %s", cases, err.c_str());
    sup_widths(B, T, src.data(), &want);
    AlignmentSupPlan ap;
    EXPECT(alignments_validate("driver: ", u, B, T, a.begin.data(), a.units.data(), a.starts.data(), a.tol, &err), "case %d: %s", cases, err.c_str());
    EXPECT(alignments_plan("driver: ", B, T, a.begin.data(), a.starts.data(), a.tol, &ap, &err), "case %d: %s", cases, err.c_str());
    const SupPlan &p = ap.plan;
    EXPECT(p.num_states == want.num_states && p.num_arcs == want.num_arcs, "case %d: %d states, %d arcs; the arrays have %d, %d", cases, p.num_states,
           p.num_arcs, want.num_states, want.num_arcs);
    EXPECT(p.max_states_per_seq == want.max_states_per_seq && p.max_arcs_per_seq == want.max_arcs_per_seq, "case %d: per sequence %d, %d; the arrays have %d, %d",
           cases, p.max_states_per_seq, p.max_arcs_per_seq, want.max_states_per_seq, want.max_arcs_per_seq);
    EXPECT(p.max_states_per_frame == want.max_states_per_frame && p.max_arcs_per_frame == want.max_arcs_per_frame,
           "case %d: per frame %d, %d; the arrays have %d, %d", cases, p.max_states_per_frame, p.max_arcs_per_frame, want.max_states_per_frame,
           want.max_arcs_per_frame);
    EXPECT(p.wide == want.wide, "case %d: wide %d", cases, (int)p.wide);
    EXPECT(p.frame_state_begin == want.frame_state_begin, "case %d: frame_state_begin", cases);
    EXPECT(ap.seq_state_begin == ssb && ap.seq_arc_begin == sab, "case %d: the begin arrays", cases);
    std::vector<int> states(B, -1), arcs(B, -1);
    EXPECT(alignment_sizes("driver: ", u, B, T, a.begin.data(), a.units.data(), a.starts.data(), a.tol, states.data(), arcs.data(), &err), "case %d: %s", cases,
           err.c_str());
    for (int s = 0; s < B; s++)
      EXPECT(states[s] == ssb[s + 1] - ssb[s] && arcs[s] == sab[s + 1] - sab[s], "case %d sequence %d: sizes %d, %d", cases, s, states[s], arcs[s]);
    for (int k = 0; k < N; k++) EXPECT(ap.lo[k] <= a.starts[k] && a.starts[k] <= ap.hi[k], "case %d unit %d: window", cases, k);
    std::printf("minibatch: %d %d %d %d %d %d %d\n", p.num_states, p.num_arcs, p.max_states_per_seq, p.max_arcs_per_seq, p.max_states_per_frame,
                p.max_arcs_per_frame, (int)p.wide);
    cases++;
  }
  std::fclose(f);
  std::printf("plans: %d minibatches\n", cases);
}

static Alignments good() {  // 3 sequences of 6 frames: 1, 3 and 2 units
  return Alignments{3, 6, 1, {0, 1, 4, 6}, {0, 1, 2, 3, 4, 0}, {0, 0, 2, 5, 0, 3}};
}

static void refusal(const Alignments &a, const char *want, int B = -1, int T = -1) {
  std::string err;
  std::vector<int> states(3), arcs(3);
  const bool ok = alignment_sizes("driver: ", unit_set(5), B < 0 ? a.B : B, T < 0 ? a.T : T, a.begin.data(), a.units.data(), a.starts.data(), a.tol,
                                  states.data(), arcs.data(), &err);
  std::printf("refusal: %s\n", err.c_str());
  EXPECT(!ok && err == std::string("driver: ") + want, "wanted '%s', got '%s'", want, err.c_str());
}

static void refusals() {
  std::string err;
  EXPECT(alignment_sizes("driver: ", unit_set(5), 3, 6, good().begin.data(), good().units.data(), good().starts.data(), 1, nullptr, nullptr, &err), "%s",
         err.c_str());
  refusal(good(), "bad arguments (num_sequences 0, frames_per_sequence 6, or a null array)", 0);
  refusal(good(), "bad arguments (num_sequences 3, frames_per_sequence 0, or a null array)", -1, 0);
  Alignments a = good();
  a.tol = -1;
  refusal(a, "tolerance -1 is negative");
  a = good();
  a.begin[0] = 1;
  refusal(a, "unit_begin must start at 0");
  a = good();
  a.begin[2] = a.begin[1];
  refusal(a, "sequence 1 has 0 units: an alignment has one at least (unit_begin must not decrease)");
  a = good();
  a.begin[2] = 0;
  refusal(a, "sequence 1 has -1 units: an alignment has one at least (unit_begin must not decrease)");
  a = good();
  a.units[5] = 5;
  refusal(a, "sequence 2 unit 1: unit 5 outside [0, 5)");
  a = good();
  a.units[0] = -1;
  refusal(a, "sequence 0 unit 0: unit -1 outside [0, 5)");
  a = good();
  a.starts[4] = 1;
  refusal(a, "sequence 2 unit 0: starts at frame 1, the first unit starts at frame 0");
  a = good();
  a.starts[3] = 2;
  refusal(a, "sequence 1 unit 2: starts at frame 2, not behind the start 2 of the unit before it");
  a = good();
  a.starts[2] = 6;
  a.starts[3] = 7;
  refusal(a, "sequence 1 unit 1: starts at frame 6, outside the 6 frames of a sequence");
}

static void capacities() {
  const Alignments a = good();
  AlignmentSupPlan ap;
  std::string err;
  EXPECT(alignments_plan("driver: ", a.B, a.T, a.begin.data(), a.starts.data(), a.tol, &ap, &err), "%s", err.c_str());
  const int NS = ap.plan.num_states, NA = ap.plan.num_arcs;
  EXPECT(sup_check_capacity("driver: ", 3, 6, ap.plan, 3, 6, NS, NA, &err), "%s", err.c_str());
  const int caps[4][4] = {{2, 6, NS, NA}, {3, 5, NS, NA}, {3, 6, NS - 1, NA}, {3, 6, NS, NA - 1}};
  const char *names[4] = {"max_sequences = 2 by 1", "max_frames = 5 by 1", "max_states", "max_arcs"};
  for (int i = 0; i < 4; i++) {
    err.clear();
    const bool ok = sup_check_capacity("driver: ", 3, 6, ap.plan, caps[i][0], caps[i][1], caps[i][2], caps[i][3], &err);
    std::printf("capacity: %s\n", err.c_str());
    EXPECT(!ok && std::strstr(err.c_str(), names[i]) && std::strstr(err.c_str(), " by 1") && !std::strncmp(err.c_str(), "driver: ", 8), "%s", err.c_str());
  }
  // the staging of the reserve holds an assign from alignments: on the host the three begins, three ints a unit and frame_state_begin; on
  // the device the two begins, three ints a unit and the four arc arrays
  const size_t N = a.units.size(), have = sup_stage_bytes(3, 6, NS, NA);
  EXPECT(sizeof(int) * (3 * 4 + 3 * N + 3 * 8) <= have && sizeof(int) * (2 * 4 + 3 * N + 4 * (size_t)NA) <= have, "%zu", have);
}

// a tolerance beyond any int sum, and the windows of an alignment whose every unit is one frame
static void windows() {
  const int T = 9;
  std::vector<int> starts(T), lo(T), hi(T);
  for (int k = 0; k < T; k++) starts[k] = k;
  alignment_windows(T, T, starts.data(), 2147483647, lo.data(), hi.data());
  for (int k = 0; k < T; k++) EXPECT(lo[k] == k && hi[k] == k, "unit %d: [%d, %d]", k, lo[k], hi[k]);
  const int two[2] = {0, 4};
  alignment_windows(2, T, two, 2147483647, lo.data(), hi.data());
  EXPECT(lo[0] == 0 && hi[0] == 0 && lo[1] == 1 && hi[1] == T - 1, "[%d, %d] [%d, %d]", lo[0], hi[0], lo[1], hi[1]);
}

int main(int argc, char **argv) {
  refusals();
  capacities();
  windows();
  if (argc > 1) from_file(argv[1]);
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
