// transcript_adapter_driver.cc -- instantiates the transcript calls of the Kaldi-side header (include/tdnnf_nnet3_adapter.h: UnitSetCreate,
// AlignGraphsAssignTranscripts, SupervisionAssignE2eTranscripts) and checks that a refusal of each C entry surfaces as an exception that
// names it.  No device is needed: each call is refused before anything is allocated or launched.  Used by
// tests/test_transcript_adapter_compile.py.
// Build: g++ -std=c++14 -I include tests/transcript_adapter_driver.cc -L tdnn-f_nas_amd -ltdnnf_hip
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
  const int pdf[2] = {0, 2}, begin[2] = {0, 2}, unit[2] = {0, 1}, optional[2] = {1, 0};
  const float logprob[2] = {-0.5f, -1.0f};
  int rc = refused("unit set", "unit_set_create: entry_pdf[1] is 2, outside [0, 2)",
                   [&] { tdnnf_adapter::UnitSetCreate(2, 2, 0, pdf, pdf, logprob, logprob, 0.0f, -1.0f); });
  rc |= refused("graphs", "align_graphs_assign_transcripts: ",
                [&] { tdnnf_adapter::AlignGraphsAssignTranscripts(nullptr, nullptr, 1, begin, unit, optional, nullptr); });
  rc |= refused("supervision", "supervision_assign_e2e_transcripts: ",
                [&] { tdnnf_adapter::SupervisionAssignE2eTranscripts(nullptr, nullptr, 1, 5, begin, unit, optional, 1.0f, nullptr); });
  // the wrappers of include/tdnnf_nnet3_components.h over vectors, on the hooks' stream
  const std::vector<int> vpdf(pdf, pdf + 2), vbegin(begin, begin + 2), vunit(unit, unit + 2), voptional(optional, optional + 2);
  const std::vector<float> vlogprob(logprob, logprob + 2);
  rc |= refused("components unit set", "unit_set_create: entry_pdf[1] is 2", [&] { tdnnf_nnet3::CreateUnitSet(2, 0, vpdf, vpdf, vlogprob, vlogprob, 0.0f, -1.0f); });
  rc |= refused("components sizes", "CreateUnitSet: the tables' sizes", [&] { tdnnf_nnet3::CreateUnitSet(2, 1, vpdf, vpdf, vlogprob, vlogprob, 0.0f, -1.0f); });
  rc |= refused("components graphs", "align_graphs_assign_transcripts: ",
                [&] { tdnnf_nnet3::AssignAlignGraphsFromTranscripts(nullptr, nullptr, vbegin, vunit, voptional); });
  rc |= refused("components supervision", "supervision_assign_e2e_transcripts: ",
                [&] { tdnnf_nnet3::AssignEnd2EndSupervisionFromTranscripts(nullptr, nullptr, 5, vbegin, vunit, voptional, 1.0f); });
  return rc;
}
