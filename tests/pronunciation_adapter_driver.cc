// pronunciation_adapter_driver.cc -- instantiates the pronunciation calls of the Kaldi-side header (include/tdnnf_nnet3_adapter.h:
// PronunciationGraphSizes, AlignGraphsAssignPronunciations, SupervisionAssignE2ePronunciations, and their wrappers over vectors in
// include/tdnnf_nnet3_components.h) and checks that a refusal of each C entry surfaces as an exception that names it.  No device is
// needed: each call is refused before anything is allocated or launched.  Used by tests/test_pronunciation_plan_cpu.py.
// Build: g++ -std=c++14 -I include tests/pronunciation_adapter_driver.cc -L tdnn-f_nas_amd -ltdnnf_hip
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
  // one transcript of two positions: [0 1] | [1], then [0]
  const int pos_begin[2] = {0, 2}, pos_optional[2] = {0, 1}, pos_alt_begin[3] = {0, 2, 3}, alt_unit_begin[4] = {0, 2, 3, 4}, alt_units[4] = {0, 1, 1, 0};
  const float alt_logprob[3] = {-0.5f, -1.0f, 0.0f};
  int states = 0, arcs = 0;
  int rc = refused("sizes", "pronunciation_graph_sizes: ", [&] {
    tdnnf_adapter::PronunciationGraphSizes(nullptr, 1, pos_begin, pos_optional, pos_alt_begin, alt_logprob, alt_unit_begin, alt_units, &states, &arcs);
  });
  rc |= refused("graphs", "align_graphs_assign_pronunciations: ", [&] {
    tdnnf_adapter::AlignGraphsAssignPronunciations(nullptr, nullptr, 1, pos_begin, pos_optional, pos_alt_begin, alt_logprob, alt_unit_begin, alt_units, nullptr);
  });
  rc |= refused("supervision", "supervision_assign_e2e_pronunciations: ", [&] {
    tdnnf_adapter::SupervisionAssignE2ePronunciations(nullptr, nullptr, 1, 5, pos_begin, pos_optional, pos_alt_begin, alt_logprob, alt_unit_begin, alt_units, 1.0f,
                                                      nullptr);
  });
  // the wrappers of include/tdnnf_nnet3_components.h over vectors, on the hooks' stream
  tdnnf_nnet3::PronunciationTranscripts t;
  t.pos_begin.assign(pos_begin, pos_begin + 2);
  t.pos_optional.assign(pos_optional, pos_optional + 2);
  t.pos_alt_begin.assign(pos_alt_begin, pos_alt_begin + 3);
  t.alt_logprob.assign(alt_logprob, alt_logprob + 3);
  t.alt_unit_begin.assign(alt_unit_begin, alt_unit_begin + 4);
  t.alt_units.assign(alt_units, alt_units + 4);
  std::vector<int> vstates, varcs;
  rc |= refused("components sizes", "pronunciation_graph_sizes: ", [&] { tdnnf_nnet3::PronunciationGraphSizes(nullptr, t, &vstates, &varcs); });
  rc |= refused("components graphs", "align_graphs_assign_pronunciations: ", [&] { tdnnf_nnet3::AssignAlignGraphsFromPronunciations(nullptr, nullptr, t); });
  rc |= refused("components supervision", "supervision_assign_e2e_pronunciations: ",
                [&] { tdnnf_nnet3::AssignEnd2EndSupervisionFromPronunciations(nullptr, nullptr, 5, t, 1.0f); });
  return rc || vstates.size() != 1 || varcs.size() != 1;
}
