// alignment_chunk_driver.cc -- the host side of tdnnf_supervision_assign_alignment_chunks (tdnn-f_nas_amd/csrc/chain_sup_alignment.h: what
// runs before anything reaches the device) as a stand-alone program, for a build under the address and undefined-behaviour sanitizers.
// Given a file of minibatches of chunks -- the utterances' alignments, the chunks and, from the statement of the lattice
// (tests/alignment_chunk_ref.py), the lattice's arrays and the units it names; tests/test_alignment_chunk_plan_cpu.py writes it -- it plans
// each from the alignments and holds every field of the plan, both begin arrays and the sizes entry's answers against what sup_validate and
// sup_widths (chain_sup_tables.h) find on the arrays; the staged slice against the named units; and, with every sequence's slice in an
// allocation of exactly its size, what the compile kernel's per-state function (ali_chunk_state, ali_chunk_frame_arcs) writes against the
// arrays, arc for arc.  Then every refusal by its message, the capacities one short, and the staging refusal of a reserve too small for a
// minibatch of one-frame chunks.  No device, no library.
// Build: g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I tdnn-f_nas_amd/csrc tests/alignment_chunk_driver.cc
#include <cmath>
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

static TranscriptUnits unit_set(int U, int context = 0) {
  TranscriptUnits u;
  u.U = U;
  u.P = 2 * U;
  u.context = context;
  u.take_logprob = u.skip_logprob = 0.f;
  return u;
}

struct Chunks {
  int B, T, tol;
  std::vector<int> begin, units, starts, utt_frames, chunk_begin;
};

// What the compile kernel does for one planned minibatch, a thread's work after the other: the frames' first arcs, then every state.
// Sequence s's slice lies in vectors of its own, so that a read beside it is a read beside an allocation.
static void compile_on_the_host(int cases, const Chunks &a, const TranscriptUnits &u, const AlignmentSupPlan &ap, const std::vector<int> &time,
                                const std::vector<float> &fin, const std::vector<int> &src, const std::vector<int> &dst, const std::vector<int> &pdf) {
  const int T = a.T, NS = ap.plan.num_states, NA = ap.plan.num_arcs;
  std::vector<int> got_time(NS, -7), got_src(NA, -7), got_dst(NA, -7), got_pdf(NA, -7), writes(NA, 0);
  std::vector<float> got_fin(NS, 7.f);
  for (int s = 0; s < a.B; s++) {
    const int q0 = ap.slice_begin[s], cnt = ap.slice_begin[s + 1] - q0, base = ap.chunk[4 * s + 3];
    const std::vector<int> unit(ap.units.begin() + q0, ap.units.begin() + q0 + cnt), lo(ap.lo.begin() + q0, ap.lo.begin() + q0 + cnt),
        hi(ap.hi.begin() + q0, ap.hi.begin() + q0 + cnt);
    const AliChunk ch = {unit.data() - base, lo.data() - base, hi.data() - base, ap.chunk[4 * s + 1], ap.chunk[4 * s], ap.chunk[4 * s + 2], T, base, cnt};
    const int s0 = ap.seq_state_begin[s], s1 = ap.seq_state_begin[s + 1], a0 = ap.seq_arc_begin[s], a1 = ap.seq_arc_begin[s + 1];
    const int *fsb = ap.plan.frame_state_begin.data() + (size_t)s * (T + 2);
    std::vector<int> fab(T + 1);
    int at = a0;
    for (int t = 0; t <= T; t++) {
      fab[t] = at;
      at += ali_chunk_frame_arcs(ch, t);
    }
    EXPECT(at == a1, "case %d sequence %d: the frames have %d arcs, the plan %d", cases, s, at - a0, a1 - a0);
    for (int g = s0; g < s1; g++) {
      const AliState st = ali_chunk_state(ch, fsb, fab.data(), s0, a0, g);
      EXPECT(st.t >= 0, "case %d sequence %d: state %d is none", cases, s, g);
      if (st.t < 0) continue;
      got_time[g] = st.t;
      got_fin[g] = st.t == T ? 0.f : -INFINITY;
      for (const AliArc &r : st.arc) {
        if (r.a < 0) continue;
        const bool inside = r.a >= a0 && r.a < a1 && r.dst >= s0 && r.dst < s1;
        EXPECT(inside, "case %d sequence %d state %d: arc %d to %d outside the sequence", cases, s, g, r.a, r.dst);
        if (!inside) continue;
        const int i = transcript_pdf_index(u, r.left, r.unit);
        got_src[r.a] = r.src;
        got_dst[r.a] = r.dst;
        got_pdf[r.a] = r.entry ? u.entry_pdf[i] : u.loop_pdf[i];
        writes[r.a]++;
      }
    }
  }
  EXPECT(got_time == time && got_fin == fin, "case %d: state_time or final_logprob", cases);
  EXPECT(got_src == src && got_dst == dst && got_pdf == pdf, "case %d: the arcs", cases);
  EXPECT(writes == std::vector<int>(NA, 1), "case %d: an arc written twice or never", cases);
}

// file: per minibatch "U context B T tolerance N NS NA", then entry_pdf and loop_pdf (U or (U + 1) * U ints each), unit_begin, units, starts,
// utt_frames, chunk_begin, per sequence the least and the largest unit its lattice names, and of the lattice seq_state_begin,
// seq_arc_begin, state_time, final_logprob, arc_src, arc_dst, arc_pdf, arc_logprob
static void from_file(const char *path) {
  FILE *f = std::fopen(path, "r");
  if (!f) {
    std::printf("FAILED to open %s\n", path);
    failures++;
    return;
  }
  Chunks a;
  int U, context, N, NS, NA, cases = 0;
  while (std::fscanf(f, "%d %d %d %d %d %d %d %d", &U, &context, &a.B, &a.T, &a.tol, &N, &NS, &NA) == 8) {
    const auto ints = [&](std::vector<int> *v, int n) {
      v->assign(n, 0);
      for (int &x : *v)
        if (std::fscanf(f, "%d", &x) != 1) failures++;
    };
    const auto floats = [&](std::vector<float> *v, int n) {
      v->assign(n, 0.f);
      for (float &x : *v) {
        if (std::fscanf(f, "%f", &x) != 1) failures++;
        if (x < -1e29f) x = -INFINITY;
      }
    };
    TranscriptUnits u = unit_set(U, context);
    ints(&u.entry_pdf, context ? (U + 1) * U : U);
    ints(&u.loop_pdf, context ? (U + 1) * U : U);
    std::vector<int> named, ssb, sab, time, src, dst, pdf;
    std::vector<float> fin, lp;
    ints(&a.begin, a.B + 1);
    ints(&a.units, N);
    ints(&a.starts, N);
    ints(&a.utt_frames, a.B);
    ints(&a.chunk_begin, a.B);
    ints(&named, 2 * a.B);
    ints(&ssb, a.B + 1);
    ints(&sab, a.B + 1);
    ints(&time, NS);
    floats(&fin, NS);
    ints(&src, NA);
    ints(&dst, NA);
    ints(&pdf, NA);
    floats(&lp, NA);
    const int B = a.B, T = a.T;
    std::string err;
    SupPlan want;
    EXPECT(sup_validate("driver: ", true, B, T, ssb.data(), sab.data(), time.data(), fin.data(), src.data(), dst.data(), pdf.data(), lp.data(), &want, &err),
           "case %d: the statement's arrays: %s", cases, err.c_str());
    sup_widths(B, T, src.data(), &want);
    AlignmentSupPlan ap;
    EXPECT(alignments_validate("driver: ", u, B, T, a.begin.data(), a.units.data(), a.starts.data(), a.tol, &err, true, a.utt_frames.data(), a.chunk_begin.data()),
           "case %d: %s", cases, err.c_str());
    EXPECT(alignment_chunks_plan("driver: ", B, T, a.begin.data(), a.units.data(), a.starts.data(), a.utt_frames.data(), a.chunk_begin.data(), a.tol, &ap, &err),
           "case %d: %s", cases, err.c_str());
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
    EXPECT(alignment_sizes("driver: ", u, B, T, a.begin.data(), a.units.data(), a.starts.data(), a.tol, states.data(), arcs.data(), &err, true,
                           a.utt_frames.data(), a.chunk_begin.data()),
           "case %d: %s", cases, err.c_str());
    for (int s = 0; s < B; s++)
      EXPECT(states[s] == ssb[s + 1] - ssb[s] && arcs[s] == sab[s + 1] - sab[s], "case %d sequence %d: sizes %d, %d", cases, s, states[s], arcs[s]);
    // the slices: in utterance coordinates, around every unit the cut lattice names, the utterance's own units and windows
    bool slices = ap.slice_begin.size() == (size_t)B + 1 && ap.chunk.size() == 4 * (size_t)B && ap.slice_begin[0] == 0 &&
                  ap.units.size() == ap.lo.size() && ap.hi.size() == ap.lo.size() && (size_t)ap.slice_begin[B] == ap.lo.size();
    EXPECT(slices, "case %d: the slices' arrays", cases);
    for (int s = 0; slices && s < B; s++) {
      const int k0 = a.begin[s], n = a.begin[s + 1] - k0, q0 = ap.slice_begin[s], cnt = ap.slice_begin[s + 1] - q0, base = ap.chunk[4 * s + 3];
      EXPECT(ap.chunk[4 * s] == a.utt_frames[s] && ap.chunk[4 * s + 1] == n && ap.chunk[4 * s + 2] == a.chunk_begin[s], "case %d sequence %d: scalars", cases, s);
      const bool inside = cnt >= 1 && base >= 0 && base + cnt <= n && base <= named[2 * s] && named[2 * s + 1] < base + cnt;
      EXPECT(inside, "case %d sequence %d: the slice [%d, %d) of %d units, the lattice names [%d, %d]", cases, s, base, base + cnt, n, named[2 * s],
             named[2 * s + 1]);
      slices = slices && inside;
      std::vector<int> lo(n), hi(n);
      alignment_windows(n, a.utt_frames[s], a.starts.data() + k0, a.tol, lo.data(), hi.data());
      for (int i = 0; inside && i < cnt; i++)
        EXPECT(ap.units[q0 + i] == a.units[k0 + base + i] && ap.lo[q0 + i] == lo[base + i] && ap.hi[q0 + i] == hi[base + i], "case %d sequence %d: staged unit %d",
               cases, s, i);
      // (the units that own a state are at most the states behind the start; a neighbour on either side)
      EXPECT(cnt <= states[s] - 1 + 2, "case %d sequence %d: %d units staged for %d states", cases, s, cnt, states[s]);
    }
    if (slices) compile_on_the_host(cases, a, u, ap, time, fin, src, dst, pdf);
    std::printf("minibatch: %d %d %d %d %d %d %d %d\n", p.num_states, p.num_arcs, p.max_states_per_seq, p.max_arcs_per_seq, p.max_states_per_frame,
                p.max_arcs_per_frame, (int)p.wide, (int)ap.lo.size());
    cases++;
  }
  std::fclose(f);
  std::printf("plans: %d minibatches\n", cases);
}

static Chunks good() {  // 3 chunks of 3 frames out of utterances of 6, 7 and 3 frames with 1, 3 and 2 units
  return Chunks{3, 3, 1, {0, 1, 4, 6}, {0, 1, 2, 3, 4, 0}, {0, 0, 2, 5, 0, 2}, {6, 7, 3}, {3, 2, 0}};
}

static void refusal(const Chunks &a, const char *want, int B = -1, int T = -1, bool no_frames = false) {
  std::string err;
  std::vector<int> states(3), arcs(3);
  const bool ok = alignment_sizes("driver: ", unit_set(5), B < 0 ? a.B : B, T < 0 ? a.T : T, a.begin.data(), a.units.data(), a.starts.data(), a.tol,
                                  states.data(), arcs.data(), &err, true, no_frames ? nullptr : a.utt_frames.data(), a.chunk_begin.data());
  std::printf("refusal: %s\n", err.c_str());
  EXPECT(!ok && err == std::string("driver: ") + want, "wanted '%s', got '%s'", want, err.c_str());
}

static void refusals() {
  std::string err;
  const Chunks g = good();
  EXPECT(alignment_sizes("driver: ", unit_set(5), 3, 3, g.begin.data(), g.units.data(), g.starts.data(), 1, nullptr, nullptr, &err, true, g.utt_frames.data(),
                         g.chunk_begin.data()),
         "%s", err.c_str());
  // what alignments_validate refuses, with the utterance's frames in place of T
  refusal(good(), "bad arguments (num_sequences 0, frames_per_sequence 3, or a null array)", 0);
  refusal(good(), "bad arguments (num_sequences 3, frames_per_sequence 0, or a null array)", -1, 0);
  refusal(good(), "bad arguments (num_sequences 3, frames_per_sequence 3, or a null array)", -1, -1, true);
  Chunks a = good();
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
  a.starts[3] = 7;  // (frame 5, beyond T = 3, is fine: the utterance has 7)
  refusal(a, "sequence 1 unit 2: starts at frame 7, outside the 7 frames of a sequence");
  // what the chunks add
  a = good();
  a.utt_frames[0] = 0;
  refusal(a, "sequence 0: an utterance of 0 frames: it has one at least");
  a = good();
  a.chunk_begin[1] = -1;
  refusal(a, "sequence 1: the chunk begins at frame -1, before the utterance");
  a = good();
  a.chunk_begin[2] = 1;
  refusal(a, "sequence 2: the chunk of 3 frames from frame 1 ends behind the 3 frames of the utterance");
  a = good();
  a.chunk_begin[0] = 2147483647;  // (no sum overflows)
  refusal(a, "sequence 0: the chunk of 3 frames from frame 2147483647 ends behind the 6 frames of the utterance");
}

static AlignmentSupPlan plan_of(const Chunks &a) {
  AlignmentSupPlan ap;
  std::string err;
  EXPECT(alignments_validate("driver: ", unit_set(5), a.B, a.T, a.begin.data(), a.units.data(), a.starts.data(), a.tol, &err, true, a.utt_frames.data(),
                             a.chunk_begin.data()),
         "%s", err.c_str());
  EXPECT(alignment_chunks_plan("driver: ", a.B, a.T, a.begin.data(), a.units.data(), a.starts.data(), a.utt_frames.data(), a.chunk_begin.data(), a.tol, &ap, &err),
         "%s", err.c_str());
  return ap;
}

static void capacities() {
  const AlignmentSupPlan ap = plan_of(good());
  std::string err;
  const int NS = ap.plan.num_states, NA = ap.plan.num_arcs;
  EXPECT(sup_check_capacity("driver: ", 3, 3, ap.plan, 3, 3, NS, NA, &err), "%s", err.c_str());
  const int caps[4][4] = {{2, 3, NS, NA}, {3, 2, NS, NA}, {3, 3, NS - 1, NA}, {3, 3, NS, NA - 1}};
  const char *names[4] = {"max_sequences = 2 by 1", "max_frames = 2 by 1", "max_states", "max_arcs"};
  for (int i = 0; i < 4; i++) {
    err.clear();
    const bool ok = sup_check_capacity("driver: ", 3, 3, ap.plan, caps[i][0], caps[i][1], caps[i][2], caps[i][3], &err);
    std::printf("capacity: %s\n", err.c_str());
    EXPECT(!ok && std::strstr(err.c_str(), names[i]) && std::strstr(err.c_str(), " by 1") && !std::strncmp(err.c_str(), "driver: ", 8), "%s", err.c_str());
  }
  EXPECT(alignment_chunks_fit_staging("driver: ", 3, ap, sup_stage_bytes(3, 3, NS, NA), &err), "%s", err.c_str());
}

// One-frame chunks out of the middle of utterances of one-frame units at tolerance 0: 2 states, 1 arc and 3 staged units a sequence.  A
// reserve of exactly their states and arcs has too little staging; the refusal names the shortfall, and a reserve with that much more fits.
static void staging() {
  const int B = 8, Tu = 9;
  Chunks a{B, 1, 0, {0}, {}, {}, {}, {}};
  for (int s = 0; s < B; s++) {
    for (int k = 0; k < Tu; k++) {
      a.units.push_back(k % 5);
      a.starts.push_back(k);
    }
    a.begin.push_back((int)a.units.size());
    a.utt_frames.push_back(Tu);
    a.chunk_begin.push_back(4);
  }
  const AlignmentSupPlan ap = plan_of(a);
  const int NS = ap.plan.num_states, NA = ap.plan.num_arcs;
  EXPECT(NS == 2 * B && NA == B && ap.lo.size() == 3 * (size_t)B, "%d states, %d arcs, %zu staged units", NS, NA, ap.lo.size());
  std::string err;
  EXPECT(sup_check_capacity("driver: ", B, 1, ap.plan, B, 1, NS, NA, &err), "%s", err.c_str());
  const size_t have = sup_stage_bytes(B, 1, NS, NA);
  // on the host 2 (B + 1) + 9 B + 4 B + (B + 1) + 3 B ints, on the device 2 (B + 1) + 9 B + 4 B + 4 B
  const size_t need = sizeof(int) * (2 * (B + 1) + 13 * B + (B + 1) + 3 * B);
  EXPECT(need > have && need > sizeof(int) * (2 * (B + 1) + 13 * B + 4 * B), "%zu %zu", need, have);
  const bool ok = alignment_chunks_fit_staging("driver: ", B, ap, have, &err);
  std::printf("staging: %s\n", err.c_str());
  char want[256];
  std::snprintf(want, sizeof(want), "driver: the chunks' %d staged units need %zu bytes of staging, the supervision has %zu: short by %zu", 3 * B, need, have,
                need - have);
  EXPECT(!ok && !std::strncmp(err.c_str(), want, std::strlen(want)), "wanted '%s', got '%s'", want, err.c_str());
  const int more = (int)((need - have + 7) / 8);  // states, 8 bytes each
  EXPECT(alignment_chunks_fit_staging("driver: ", B, ap, sup_stage_bytes(B, 1, NS + more, NA), &err), "%s", err.c_str());
  EXPECT(!alignment_chunks_fit_staging("driver: ", B, ap, sup_stage_bytes(B, 1, NS + more - 1, NA), &err), "one state less still fits");
}

int main(int argc, char **argv) {
  refusals();
  capacities();
  staging();
  if (argc > 1) from_file(argv[1]);
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
