// chunk_input_adapter_driver.cc -- instantiates the chunk-input calls of the Kaldi-side header (include/tdnnf_nnet3_adapter.h:
// ChunkInputCreate, ChunkInputGather; their forms over vectors in include/tdnnf_nnet3_components.h) against a stub of CuMatrixBase<float> and checks that a refusal of each C entry surfaces as an
// exception that names it.  No device is needed: each call is refused before anything is allocated or launched.  Used by
// tests/test_chunk_input_adapter_compile.py.
// Build: g++ -std=c++14 -I include tests/chunk_input_adapter_driver.cc -L tdnn-f_nas_amd -ltdnnf_hip
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "tdnnf_nnet3_adapter.h"
#include "tdnnf_nnet3_components.h"

struct MatStub {  // what the adapter needs of a CuMatrixBase<float>
  std::vector<float> v;
  int r, c;
  MatStub(int rows, int cols) : v((size_t)rows * cols), r(rows), c(cols) {}
  const float *Data() const { return v.data(); }
  int NumRows() const { return r; }
  int NumCols() const { return c; }
  int Stride() const { return c; }
};

template <class Call>
static int refused(const char *what, const char *names, Call call) {
  try {
    call();
  } catch (const std::runtime_error &e) {
    std::printf("%s: %s\n", what, e.what());
    return std::strstr(e.what(), names) ? 0 : 1;
  }
  std::printf("%s: no exception\n", what);
  return 1;
}

int main() {
  const int seq_utt[2] = {0, 1}, chunk_begin[2] = {0, 2}, frames[2] = {13, 30}, rows[2] = {1, 2};
  MatStub feats(43, 8), ivectors(3, 4), feats_out(42, 8), ivectors_out(2, 4);
  int rc = refused("create", "chunk_input_create: bad arguments (max_sequences 0)", [&] { tdnnf_adapter::ChunkInputCreate(0); });
  rc |= refused("gather", "chunk_input_gather: null handle", [&] {
    tdnnf_adapter::ChunkInputGather(nullptr, -5, 21, 3, 4, 2, seq_utt, chunk_begin, 0, 2, frames, feats, rows, &ivectors, 10, &feats_out, &ivectors_out, nullptr);
  });
  rc |= refused("gather without i-vectors", "chunk_input_gather: null handle", [&] {
    tdnnf_adapter::ChunkInputGather<MatStub>(nullptr, -5, 21, 3, 4, 2, seq_utt, chunk_begin, 0, 2, frames, feats, nullptr, nullptr, 10, &feats_out, nullptr, nullptr);
  });
  rc |= refused("gather without an output", "ChunkInputGather needs feats_out", [&] {
    tdnnf_adapter::ChunkInputGather<MatStub>(nullptr, -5, 21, 3, 4, 2, seq_utt, chunk_begin, 0, 2, frames, feats, rows, &ivectors, 10, nullptr, &ivectors_out, nullptr);
  });
  // the wrappers of include/tdnnf_nnet3_components.h over vectors, on the hooks' stream
  namespace n3 = tdnnf_nnet3;
  const std::vector<int> vutt(seq_utt, seq_utt + 2), vbegin(chunk_begin, chunk_begin + 2), vframes(frames, frames + 2), vrows(rows, rows + 2);
  n3::CuMatrixBase cf(feats.v.data(), 43, 8, 8), ci(ivectors.v.data(), 3, 4, 4), cfo(feats_out.v.data(), 42, 8, 8), cio(ivectors_out.v.data(), 2, 4, 4);
  rc |= refused("components create", "chunk_input_create: bad arguments (max_sequences -1)", [&] { n3::NewChunkInput(-1); });
  rc |= refused("components gather", "chunk_input_gather: null handle",
                [&] { n3::GatherChunkInput(nullptr, -5, 21, 3, 4, vutt, vbegin, 0, vframes, cf, vrows, &ci, 10, &cfo, &cio); });
  rc |= refused("components lengths", "one entry a sequence",
                [&] { n3::GatherChunkInput(nullptr, -5, 21, 3, 4, vutt, std::vector<int>(1, 0), 0, vframes, cf, vrows, &ci, 10, &cfo, &cio); });
  // the host-only plan through the same header's C declarations: a refusal names the sequence
  int table[8];
  if (tdnnf_chunk_input_plan(3, 4, 2, seq_utt, chunk_begin, 0, 2, frames, rows, 10, table) != TDNNF_OK || table[4] != 13 || table[6] != 6 || table[7] != 2) rc |= 1;
  const int late[2] = {0, 7};
  if (tdnnf_chunk_input_plan(3, 4, 2, seq_utt, late, 0, 2, frames, rows, 10, table) != TDNNF_EINVAL || !std::strstr(tdnnf_last_error(), "sequence 1: the chunk of 4 frames from frame 7"))
    rc |= 1;
  std::printf("plan: %s\n", tdnnf_last_error());
  return rc;
}
