// sparse_driver.cc -- instantiates the two AlignPosteriorsSparse of the Kaldi-side headers (include/tdnnf_nnet3_adapter.h: the template over a
// CuMatrixBase; include/tdnnf_nnet3_components.h: the wrapper that sizes its Scratch), which tests/adapter_driver.cc does not reach, and
// checks that a refusal of the C entry surfaces as an exception that names it.  No device is needed: a call without graphs is refused before
// anything is launched.  Used by tests/test_sparse_adapter_compile.py.
// Build: g++ -std=c++14 -I include tests/sparse_driver.cc -L tdnn-f_nas_amd -ltdnnf_hip
#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "tdnnf_nnet3_adapter.h"
#include "tdnnf_nnet3_components.h"

template <class Call>
static int refused(const char *what, Call call) {
  try {
    call();
  } catch (const std::runtime_error &e) {
    std::printf("%s: %s\n", what, e.what());
    return std::strstr(e.what(), "align_posteriors_sparse: ") ? 0 : 1;
  }
  std::printf("%s: no exception\n", what);
  return 1;
}

int main() {
  tdnnf_nnet3::CuMatrixBase y(nullptr, 0, 0, 0);
  const int frames[2] = {3, 4}, rows[2] = {0, 3};
  int rc = refused("adapter", [&] {
    tdnnf_adapter::AlignPosteriorsSparse(nullptr, 2, nullptr, frames, rows, 1, y, 1.0f, 1.0f, 0.01f, 16, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr);
  });
  tdnnf_nnet3::Scratch workspace;  // (a refused call asks for 0 bytes: no allocator hook is needed)
  rc |= refused("components", [&] {
    tdnnf_nnet3::AlignPosteriorsSparse(nullptr, 2, nullptr, frames, rows, y, 1.0f, 1.0f, 0.01f, 16, nullptr, nullptr, nullptr, nullptr, &workspace);
  });
  return rc;
}
