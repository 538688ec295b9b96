// supervision_adapter_driver.cc -- instantiates the reusable-supervision calls of the Kaldi-side headers (include/tdnnf_nnet3_adapter.h:
// SupervisionReserve, SupervisionAssign; include/tdnnf_nnet3_components.h: ReserveSupervision, AssignSupervision) and checks that a refusal
// of each C entry surfaces as an exception that names it.  No device is needed: each call is refused before anything is allocated or
// launched.  Used by tests/test_supervision_adapter_compile.py.
// Build: g++ -std=c++14 -I include tests/supervision_adapter_driver.cc -L tdnn-f_nas_amd -ltdnnf_hip
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
  const int state_begin[2] = {0, 2}, arc_begin[2] = {0, 1}, time[2] = {0, 1}, src[1] = {0}, dst[1] = {1}, pdf[1] = {3};
  const float fin[2] = {-1e30f, 0.0f}, lp[1] = {-0.5f};
  int rc = refused("reserve", "supervision_reserve: bad arguments", [&] { tdnnf_adapter::SupervisionReserve(0, 10, 100, 100); });
  rc |= refused("reserve states", "supervision_reserve: max_states 3 is below max_sequences 4", [&] { tdnnf_adapter::SupervisionReserve(4, 10, 3, 100); });
  rc |= refused("assign", "supervision_assign: null supervision",
                [&] { tdnnf_adapter::SupervisionAssign(nullptr, 1, 1, state_begin, arc_begin, time, fin, src, dst, pdf, lp, 1.0f, nullptr); });
  // the wrappers of include/tdnnf_nnet3_components.h over vectors, on the hooks' stream
  const std::vector<int> vsb(state_begin, state_begin + 2), vab(arc_begin, arc_begin + 2), vtime(time, time + 2), vsrc(src, src + 1), vdst(dst, dst + 1),
      vpdf(pdf, pdf + 1);
  const std::vector<float> vfin(fin, fin + 2), vlp(lp, lp + 1);
  rc |= refused("components reserve", "supervision_reserve: bad arguments", [&] { tdnnf_nnet3::ReserveSupervision(2, 0, 100, 100); });
  rc |= refused("components assign", "supervision_assign: null supervision",
                [&] { tdnnf_nnet3::AssignSupervision(nullptr, 1, 1, vsb, vab, vtime, vfin, vsrc, vdst, vpdf, vlp, 1.0f); });
  return rc;
}
