// label_driver.cc -- instantiates the labelled entries of the Kaldi-side headers (include/tdnnf_nnet3_adapter.h: the templates over a
// CuMatrixBase; include/tdnnf_nnet3_components.h: the wrappers that size their Scratch) -- AlignBestPathLabels, AlignLabelPosteriorsCompact
// and AlignLabelPosteriorsSparse -- and checks that a refusal of the C entry surfaces as an exception that names it.  No device is needed:
// a label entry refuses a handle that carries no labels -- here no handle at all, which the same check turns away (a handle of
// tdnnf_align_graphs_create needs a device; tests/test_gpu_align_labels.py makes one) -- before anything is launched.
// Used by tests/test_label_adapter_compile.py.
// Build: g++ -std=c++14 -I include tests/label_driver.cc -L tdnn-f_nas_amd -ltdnnf_hip
#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "tdnnf_nnet3_adapter.h"
#include "tdnnf_nnet3_components.h"

template <class Call>
static int refused(const char *what, const char *name, Call call) {
  try {
    call();
  } catch (const std::runtime_error &e) {
    std::printf("%s: %s\n", what, e.what());
    return std::strstr(e.what(), name) ? 0 : 1;
  }
  std::printf("%s: no exception\n", what);
  return 1;
}

int main() {
  tdnnf_nnet3::CuMatrixBase y(nullptr, 0, 0, 0);
  const int frames[2] = {3, 4}, rows[2] = {0, 3};
  tdnnf_nnet3::Scratch workspace;  // (a refused call asks for 0 bytes: no allocator hook is needed)
  int rc = refused("adapter best path", "align_best_path_labels: ", [&] {
    tdnnf_adapter::AlignBestPathLabels(nullptr, 2, nullptr, frames, rows, 1, y, 1.0f, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr);
  });
  rc |= refused("components best path", "align_best_path_labels: ", [&] {
    tdnnf_nnet3::AlignBestPathLabels(nullptr, 2, nullptr, frames, rows, y, 1.0f, nullptr, nullptr, nullptr, nullptr, &workspace);
  });
  rc |= refused("adapter compact", "align_label_posteriors_compact: ", [&] {
    tdnnf_adapter::AlignLabelPosteriorsCompact(nullptr, 2, nullptr, frames, rows, 1, y, 1.0f, 1.0f, nullptr, 0, nullptr, nullptr, 0, nullptr);
  });
  rc |= refused("components compact", "align_label_posteriors_compact: ", [&] {
    tdnnf_nnet3::AlignLabelPosteriorsCompact(nullptr, 2, nullptr, frames, rows, y, 1.0f, 1.0f, nullptr, 0, nullptr, &workspace);
  });
  rc |= refused("adapter sparse", "align_label_posteriors_sparse: ", [&] {
    tdnnf_adapter::AlignLabelPosteriorsSparse(nullptr, 2, nullptr, frames, rows, 1, y, 1.0f, 1.0f, 0.01f, 16, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                                              nullptr);
  });
  rc |= refused("components sparse", "align_label_posteriors_sparse: ", [&] {
    tdnnf_nnet3::AlignLabelPosteriorsSparse(nullptr, 2, nullptr, frames, rows, y, 1.0f, 1.0f, 0.01f, 16, nullptr, nullptr, nullptr, nullptr, &workspace);
  });
  return rc;
}
