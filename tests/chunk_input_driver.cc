// chunk_input_driver.cc -- the host half of the chunk minibatch inputs (tdnn-f_nas_amd/csrc/chunk_input_plan.h: the checks and the table,
// what runs before anything reaches the device) as a stand-alone program, for a build under the address and undefined-behaviour
// sanitizers.  Every array lives in a heap block of exactly its size, so a read or a write beyond it would be reported.  It reads the
// minibatches tests/test_chunk_input_plan_cpu.py writes -- per case a line of scalars, then seq_utt, chunk_begin, frames, ivector_rows and
// the table of tests/chunk_input_ref.py -- holds the plan against that table, and runs every refusal on arrays of exact size.  No device, no
// library.
// Build: g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I tdnn-f_nas_amd/csrc tests/chunk_input_driver.cc
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "chunk_input_plan.h"

using namespace tdnnf;

static int failures = 0;
#define EXPECT(cond, ...)                \
  do {                                   \
    if (!(cond)) {                       \
      std::printf("FAILED %s: ", #cond); \
      std::printf(__VA_ARGS__);          \
      std::printf("\n");                 \
      failures++;                        \
    }                                    \
  } while (0)

static std::vector<int> ints(std::istream &in, int n) {
  std::vector<int> v(n);
  for (int &x : v) in >> x;
  return v;
}

static int plans(const char *path) {
  std::ifstream in(path);
  int cases = 0, fsf, T, B, U, shift, period, has_rows;
  while (in >> fsf >> T >> B >> U >> shift >> period >> has_rows) {
    const std::vector<int> utt = ints(in, B), begin = ints(in, B), frames = ints(in, U), rows = ints(in, has_rows ? U : 0), want = ints(in, kChunkTab * B);
    std::vector<int> got(kChunkTab * B, -7);
    ChunkInputRows r{-1, -1};
    std::string err;
    const bool use_iv = period <= 0 || has_rows;
    const bool ok = chunk_input_plan("driver: ", fsf, T, B, utt.data(), begin.data(), shift, U, frames.data(), use_iv, has_rows ? rows.data() : nullptr, period,
                                     got.data(), &r, &err);
    EXPECT(ok && err.empty(), "case %d: %s", cases, err.c_str());
    EXPECT(got == want, "case %d: the table differs", cases);
    long long sumT = 0, sumR = 0;
    for (int u = 0; u < U; u++) {
      sumT += frames[u];
      sumR += use_iv ? (period > 0 ? rows[u] : 1) : 0;
    }
    EXPECT(r.feat_rows == sumT && r.ivector_rows == sumR, "case %d: %lld %lld", cases, r.feat_rows, r.ivector_rows);
    cases++;
  }
  std::printf("plans: %d minibatches\n", cases);
  return cases;
}

static void refusals() {
  // three utterances of 13, 30 and 12 frames at fsf 3: O = 5, 10, 4; chunks of T = 4
  const std::vector<int> frames = {13, 30, 12}, rows = {1, 2, 3}, utt = {0, 1, 2}, begin = {1, 6, 0};
  const auto run = [&](const char *want, int fsf, int T, std::vector<int> u, std::vector<int> o, int shift, std::vector<int> f, bool use_iv,
                       const std::vector<int> *r, int period) {
    std::vector<int> table(kChunkTab * u.size(), -7);
    std::string err;
    const bool ok = chunk_input_plan("driver: ", fsf, T, (int)u.size(), u.data(), o.data(), shift, (int)f.size(), f.data(), use_iv, r ? r->data() : nullptr, period,
                                     table.data(), nullptr, &err);
    EXPECT(!ok && err.find(want) != std::string::npos, "wanted \"%s\", got %d \"%s\"", want, (int)ok, err.c_str());
    for (int x : table) EXPECT(x == -7, "a refused plan wrote the table");
    std::printf("refusal: %s\n", err.c_str());
  };
  const auto at = [](std::vector<int> v, int i, int x) {
    v[i] = x;
    return v;
  };
  run("driver: sequence 1: the chunk begins at frame -1", 3, 4, utt, at(begin, 1, -1), 0, frames, true, &rows, 10);
  run("driver: sequence 0: the chunk of 4 frames from frame 2 ends behind the 5 output frames of the utterance", 3, 4, utt, at(begin, 0, 2), 0, frames, true, &rows, 10);
  run("driver: sequence 2: utterance 3 outside [0, 3)", 3, 4, at(utt, 2, 3), begin, 0, frames, true, &rows, 10);
  run("driver: sequence 0: utterance -1 outside [0, 3)", 3, 4, at(utt, 0, -1), begin, 0, frames, true, &rows, 10);
  run("driver: utterance 1 has 0 frames", 3, 4, utt, begin, 0, at(frames, 1, 0), true, &rows, 10);
  run("driver: frame_shift 3: its magnitude must be below frame_subsampling 3", 3, 4, utt, begin, 3, frames, true, &rows, 10);
  run("driver: frame_shift -3: its magnitude must be below frame_subsampling 3", 3, 4, utt, begin, -3, frames, true, &rows, 10);
  const std::vector<int> no_rows = at(rows, 2, 0);
  run("driver: utterance 2 has no i-vector rows (0)", 3, 4, utt, begin, 0, frames, true, &no_rows, 10);
  run("driver: ivector_period 10 > 0 needs ivector_rows_host", 3, 4, utt, begin, 0, frames, true, nullptr, 10);
  run("driver: 0 sequences", 3, 4, {}, {}, 0, frames, true, &rows, 10);
  run("driver: frame_subsampling 0 and frames_per_sequence 4 must be positive", 0, 4, utt, begin, 0, frames, true, &rows, 10);
  // ... and what is no refusal: without i-vectors the row counts are not read, and one row an utterance needs none
  std::vector<int> table(kChunkTab * 3);
  std::string err;
  EXPECT(chunk_input_plan("driver: ", 3, 4, 3, utt.data(), begin.data(), 2, 3, frames.data(), false, nullptr, 10, table.data(), nullptr, &err), "%s", err.c_str());
  EXPECT(table[3] == 0 && table[7] == 0 && table[11] == 0 && table[2] == 1 && table[6] == 16 && table[10] == -2, "%d %d %d", table[2], table[6], table[10]);
  EXPECT(chunk_input_plan("driver: ", 3, 4, 3, utt.data(), begin.data(), 0, 3, frames.data(), true, nullptr, 0, table.data(), nullptr, &err), "%s", err.c_str());
  EXPECT(table[3] == 0 && table[7] == 1 && table[11] == 2 && table[4] == 13 && table[8] == 43, "%d %d %d", table[3], table[7], table[11]);
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  if (plans(argv[1]) == 0) failures++;
  refusals();
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
