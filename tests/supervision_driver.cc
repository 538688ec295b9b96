// supervision_driver.cc -- the host side of tdnnf_supervision_assign (tdnn-f_nas_amd/csrc/chain_sup_tables.h: what runs before anything
// reaches the device) as a stand-alone program, for a build under the address and undefined-behaviour sanitizers.  It validates a minibatch
// it makes itself against loops written from the definition, runs every refusal of tdnnf_supervision_create and each capacity one short,
// and, given a file of minibatches (tests/test_supervision_adapter_compile.py writes them from synth.py), prints the widths and
// frame_state_begin of each for the test to hold against the numpy statement (tests/supervision_tables_ref.py).  No device, no library.
// Build: g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I tdnn-f_nas_amd/csrc tests/supervision_driver.cc
#include <cstdio>
#include <cstring>

#include "chain_sup_tables.h"

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

struct Batch {
  int B, T;
  std::vector<int> ssb, sab, time, src, dst, pdf;
  std::vector<float> fin, lp;
};

// B sequences of T frames; frame t of sequence s has 1 + (s + t) % width states (frame 0: one), fully connected to the next frame's
static Batch made(int B, int T, int width) {
  Batch b;
  b.B = B;
  b.T = T;
  b.ssb.push_back(0);
  b.sab.push_back(0);
  for (int s = 0; s < B; s++) {
    std::vector<int> first(T + 2);
    int n = (int)b.time.size();
    for (int t = 0; t <= T; t++) {
      first[t] = n;
      const int c = t == 0 ? 1 : 1 + (s + t) % width;
      for (int i = 0; i < c; i++) {
        b.time.push_back(t);
        b.fin.push_back(t == T ? 0.0f : -1e30f);
      }
      n += c;
    }
    first[T + 1] = n;
    for (int t = T - 1; t >= 0; t--)  // (arcs in an order that is neither by source nor by destination)
      for (int i = first[t]; i < first[t + 1]; i++)
        for (int j = first[t + 1]; j < first[t + 2]; j++) {
          b.src.push_back(i);
          b.dst.push_back(j);
          b.pdf.push_back((3 * i + j) % 7);
          b.lp.push_back(-0.125f * ((i + j) % 5));
        }
    b.ssb.push_back(n);
    b.sab.push_back((int)b.src.size());
  }
  return b;
}

static bool validate(const Batch &b, SupPlan *p, std::string *err, int B = -1, int T = -1) {
  return sup_validate("driver: ", true, B < 0 ? b.B : B, T < 0 ? b.T : T, b.ssb.data(), b.sab.data(), b.time.data(), b.fin.data(), b.src.data(), b.dst.data(),
                      b.pdf.data(), b.lp.data(), p, err);
}

static void plans() {
  int cases = 0;
  for (int B = 1; B <= 4; B++)
    for (int T = 1; T <= 9; T += 2)
      for (int width = 1; width <= 23; width += 11) {
        const Batch b = made(B, T, width);
        SupPlan p;
        std::string err;
        EXPECT(validate(b, &p, &err), "B %d T %d width %d: %s", B, T, width, err.c_str());
        sup_widths(B, T, b.src.data(), &p);
        int states = 0, arcs = 0, seq = 0;
        for (int s = 0; s < B; s++) {
          seq = std::max(seq, b.ssb[s + 1] - b.ssb[s]);
          for (int t = 0; t <= T + 1; t++) {
            int first = b.ssb[s + 1], n = 0, leaving = 0;
            for (int i = b.ssb[s + 1] - 1; i >= b.ssb[s]; i--)
              if (b.time[i] >= t) first = i;
            EXPECT(p.frame_state_begin[(size_t)s * (T + 2) + t] == first, "B %d T %d width %d sequence %d frame %d", B, T, width, s, t);
            for (int i = b.ssb[s]; i < b.ssb[s + 1]; i++) n += b.time[i] == t ? 1 : 0;
            for (int a = b.sab[s]; a < b.sab[s + 1]; a++) leaving += b.time[b.src[a]] == t ? 1 : 0;
            states = std::max(states, n);
            arcs = std::max(arcs, leaving);
          }
        }
        EXPECT(p.num_states == b.ssb[B] && p.num_arcs == b.sab[B] && p.max_states_per_seq == seq && p.max_states_per_frame == states &&
                   p.max_arcs_per_frame == arcs && p.wide == ((long long)b.ssb[B] > (long long)B * 4 * (T + 1)),
               "B %d T %d width %d: %d %d %d %d %d %d", B, T, width, p.num_states, p.num_arcs, p.max_states_per_seq, p.max_states_per_frame,
               p.max_arcs_per_frame, (int)p.wide);
        cases++;
      }
  std::printf("plans: %d minibatches\n", cases);
  EXPECT(cases == 60, "%d", cases);
}

static void refusal(const Batch &b, const char *want, int B = -1, int T = -1) {
  SupPlan p;
  std::string err;
  const bool ok = validate(b, &p, &err, B, T);
  std::printf("refusal: %s\n", err.c_str());
  EXPECT(!ok && err == std::string("driver: ") + want, "wanted '%s', got '%s'", want, err.c_str());
}

static void refusals() {
  const Batch good = made(3, 4, 3);
  SupPlan p;
  std::string err;
  EXPECT(validate(good, &p, &err), "%s", err.c_str());
  const int s1 = good.ssb[1];
  refusal(good, "bad arguments", 0);
  refusal(good, "bad arguments", -1, 0);
  Batch b = good;
  b.time[s1] = 1;
  refusal(b, "sequence 1 must start with its time-0 start state");
  b = good;
  b.ssb[2] = b.ssb[1];
  refusal(b, "sequence 1 must start with its time-0 start state");
  b = good;
  b.time[s1 + 2] = 0;
  refusal(b, "states must be sorted by time");
  b = good;
  b.time.back() = good.T + 1;
  refusal(b, "states must be sorted by time");
  b = good;
  b.time[1] = 0;
  refusal(b, "exactly one time-0 state per sequence");
  b = good;
  b.src[0] = s1;
  refusal(b, "arc 0 must advance exactly one frame inside its sequence");
  b = good;
  b.dst[2] = -1;
  refusal(b, "arc 2 must advance exactly one frame inside its sequence");
  b = good;
  b.pdf[1] = -1;
  refusal(b, "arc 1 must advance exactly one frame inside its sequence");
  b = good;
  b.dst[0] = b.src[0];
  refusal(b, "arc 0 must advance exactly one frame inside its sequence");
  // on top of tdnnf_supervision_create's: begin arrays it would read out of bounds with
  b = good;
  b.sab[0] = 1;
  refusal(b, "seq_state_begin and seq_arc_begin must start at 0");
  b = good;
  std::swap(b.sab[1], b.sab[2]);
  refusal(b, "sequence 1 has a negative arc count");
}

static void capacities() {
  const Batch b = made(3, 4, 3);
  SupPlan p;
  std::string err;
  EXPECT(validate(b, &p, &err), "%s", err.c_str());
  const int NS = p.num_states, NA = p.num_arcs;
  EXPECT(sup_check_capacity("driver: ", 3, 4, p, 3, 4, NS, NA, &err), "%s", err.c_str());
  const int caps[4][4] = {{2, 4, NS, NA}, {3, 3, NS, NA}, {3, 4, NS - 1, NA}, {3, 4, NS, NA - 1}};
  const char *names[4] = {"max_sequences = 2 by 1", "max_frames = 3 by 1", "max_states", "max_arcs"};
  for (int i = 0; i < 4; i++) {
    err.clear();
    const bool ok = sup_check_capacity("driver: ", 3, 4, p, caps[i][0], caps[i][1], caps[i][2], caps[i][3], &err);
    std::printf("capacity: %s\n", err.c_str());
    EXPECT(!ok && std::strstr(err.c_str(), names[i]) && std::strstr(err.c_str(), " by 1") && !std::strncmp(err.c_str(), "driver: ", 8), "%s", err.c_str());
  }
  EXPECT(sup_stage_bytes(3, 4, NS, NA) == sizeof(int) * (8 + 18 + 2 * (size_t)NS + 4 * (size_t)NA), "%zu", sup_stage_bytes(3, 4, NS, NA));
}

// file: per minibatch "B T NS NA", then seq_state_begin, seq_arc_begin, state_time, final_logprob, arc_src, arc_dst, arc_pdf, arc_logprob
static void from_file(const char *path) {
  FILE *f = std::fopen(path, "r");
  if (!f) {
    std::printf("FAILED to open %s\n", path);
    failures++;
    return;
  }
  Batch b;
  int NS, NA;
  while (std::fscanf(f, "%d %d %d %d", &b.B, &b.T, &NS, &NA) == 4) {
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
    ints(&b.ssb, b.B + 1);
    ints(&b.sab, b.B + 1);
    ints(&b.time, NS);
    floats(&b.fin, NS);
    ints(&b.src, NA);
    ints(&b.dst, NA);
    ints(&b.pdf, NA);
    floats(&b.lp, NA);
    SupPlan p;
    std::string err;
    EXPECT(validate(b, &p, &err), "%s", err.c_str());
    sup_widths(b.B, b.T, b.src.data(), &p);
    std::printf("minibatch: %d %d %d %d %d %d\nframes:", p.num_states, p.num_arcs, p.max_states_per_seq, p.max_states_per_frame, p.max_arcs_per_frame,
                (int)p.wide);
    for (int x : p.frame_state_begin) std::printf(" %d", x);
    std::printf("\n");
  }
  std::fclose(f);
}

int main(int argc, char **argv) {
  plans();
  refusals();
  capacities();
  if (argc > 1) from_file(argv[1]);
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
