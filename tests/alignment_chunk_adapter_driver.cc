// alignment_chunk_adapter_driver.cc -- instantiates the alignment-chunk calls of the Kaldi-side headers (include/tdnnf_nnet3_adapter.h:
// AlignmentChunkSupervisionSizes, SupervisionAssignAlignmentChunks; their forms over vectors in include/tdnnf_nnet3_components.h) and
// checks that a refusal of each C entry surfaces as an exception that names it.  No device is needed: each call is refused before
// anything is allocated or launched.  Used by tests/test_alignment_chunk_adapter_compile.py.
// Build: g++ -std=c++14 -I include tests/alignment_chunk_adapter_driver.cc -L tdnn-f_nas_amd -ltdnnf_hip
#include <cstdio>
#include <cstring>
#include <stdexcept>

#include <vector>

#include "tdnnf_nnet3_adapter.h"
#include "tdnnf_nnet3_components.h"

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
  const int begin[2] = {0, 2}, unit[2] = {0, 1}, starts[2] = {0, 3}, utt_frames[1] = {9}, chunk_begin[1] = {2};
  int states[1], arcs[1];
  int rc = refused("sizes", "alignment_chunk_supervision_sizes: null unit set", [&] {
    tdnnf_adapter::AlignmentChunkSupervisionSizes(nullptr, 1, 5, begin, unit, starts, utt_frames, chunk_begin, 2, states, arcs);
  });
  rc |= refused("supervision", "supervision_assign_alignment_chunks: null supervision or null unit set", [&] {
    tdnnf_adapter::SupervisionAssignAlignmentChunks(nullptr, nullptr, 1, 5, begin, unit, starts, utt_frames, chunk_begin, 2, 1.0f, nullptr);
  });
  // the wrappers of include/tdnnf_nnet3_components.h over vectors, on the hooks' stream
  const std::vector<int> vbegin(begin, begin + 2), vunit(unit, unit + 2), vstarts(starts, starts + 2), vframes(1, 9), vchunk(1, 2);
  std::vector<int> vstates, varcs;
  rc |= refused("components sizes", "alignment_chunk_supervision_sizes: null unit set",
                [&] { tdnnf_nnet3::AlignmentChunkSupervisionSizes(nullptr, 5, vbegin, vunit, vstarts, vframes, vchunk, 2, &vstates, &varcs); });
  rc |= refused("components supervision", "supervision_assign_alignment_chunks: ",
                [&] { tdnnf_nnet3::AssignSupervisionFromAlignmentChunks(nullptr, nullptr, 5, vbegin, vunit, vstarts, vframes, vchunk, 2, 1.0f); });
  rc |= refused("components lengths", "one entry a sequence",
                [&] { tdnnf_nnet3::AssignSupervisionFromAlignmentChunks(nullptr, nullptr, 5, vbegin, vunit, vstarts, vframes, vunit, 2, 1.0f); });
  return rc;
}
