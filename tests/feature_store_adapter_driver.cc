// feature_store_adapter_driver.cc -- instantiates the feature-store calls of the Kaldi-side header (include/tdnnf_nnet3_adapter.h:
// FeatureStoreCreate, FeatureStoreAppend, FeatureStoreExpand, ChunkInputGatherStored; their forms over vectors in
// include/tdnnf_nnet3_components.h) against a stub of CuMatrixBase<float> and checks that
// a refusal of each C entry surfaces as an exception that names it; then the host-only entries through the same header's C declarations.
// No device is needed: each call is refused before anything is allocated or launched.  Used by
// tests/test_feature_store_adapter_compile.py.
// Build: g++ -std=c++14 -I include tests/feature_store_adapter_driver.cc -L tdnn-f_nas_amd -ltdnnf_hip
#include <cstdint>
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
  const int seq_utt[2] = {0, 1}, chunk_begin[2] = {0, 2}, rows[2] = {1, 2};
  MatStub ivectors(3, 4), feats_out(42, 8), ivectors_out(2, 4), expanded(43, 8);
  // a CM payload of 2 rows x 3 columns as an archive holds it: percentiles a column, bytes column-major
  const uint16_t pct[12] = {0, 100, 200, 65535, 5, 5, 5, 5, 1, 2, 3, 4};
  const uint8_t codes[6] = {0, 64, 65, 192, 193, 255};
  tdnnf_feature_payload item;
  item.format = 1, item.min_value = -2.f, item.range = 8.f, item.rows = 2, item.cols = 3, item.percentiles = pct, item.codes = codes;
  int rc = refused("create", "feature_store_create: format 4: a store holds format 1 (CM), 2 (CM2) or 3 (CM3)", [&] { tdnnf_adapter::FeatureStoreCreate(4, 8, 3, 55); });
  rc |= refused("create capacities", "feature_store_create: bad arguments (feat_dim 8, max_utterances 0, max_frames 55)",
                [&] { tdnnf_adapter::FeatureStoreCreate(1, 8, 0, 55); });
  rc |= refused("append", "feature_store_append: null handle", [&] { tdnnf_adapter::FeatureStoreAppend(nullptr, 1, &item); });
  rc |= refused("expand", "feature_store_expand: null handle", [&] { tdnnf_adapter::FeatureStoreExpand(nullptr, 2, seq_utt, &expanded, nullptr); });
  rc |= refused("expand without an output", "FeatureStoreExpand needs out", [&] { tdnnf_adapter::FeatureStoreExpand<MatStub>(nullptr, 2, seq_utt, nullptr, nullptr); });
  rc |= refused("gather", "chunk_input_gather_stored: null handle", [&] {
    tdnnf_adapter::ChunkInputGatherStored(nullptr, -5, 21, 3, 4, 2, seq_utt, chunk_begin, 0, nullptr, rows, &ivectors, 10, &feats_out, &ivectors_out, nullptr);
  });
  rc |= refused("gather without an output", "ChunkInputGatherStored needs feats_out", [&] {
    tdnnf_adapter::ChunkInputGatherStored<MatStub>(nullptr, -5, 21, 3, 4, 2, seq_utt, chunk_begin, 0, nullptr, rows, &ivectors, 10, nullptr, &ivectors_out, nullptr);
  });
  // the wrappers of include/tdnnf_nnet3_components.h over vectors, on the hooks' stream
  namespace n3 = tdnnf_nnet3;
  const std::vector<int> vutt(seq_utt, seq_utt + 2), vbegin(chunk_begin, chunk_begin + 2), vrows(rows, rows + 2);
  n3::CuMatrixBase ci(ivectors.v.data(), 3, 4, 4), cfo(feats_out.v.data(), 42, 8, 8), cio(ivectors_out.v.data(), 2, 4, 4), cex(expanded.v.data(), 43, 8, 8);
  rc |= refused("components create", "feature_store_create: bad arguments (feat_dim 0, max_utterances 3, max_frames 55)", [&] { n3::NewFeatureStore(2, 0, 3, 55); });
  rc |= refused("components append", "feature_store_append: null handle", [&] { n3::AppendFeatureStore(nullptr, std::vector<tdnnf_feature_payload>(1, item)); });
  rc |= refused("components expand", "feature_store_expand: null handle", [&] { n3::ExpandFeatureStore(nullptr, vutt, &cex); });
  rc |= refused("components gather", "chunk_input_gather_stored: null handle",
                [&] { n3::GatherStoredChunkInput(nullptr, -5, 21, 3, 4, vutt, vbegin, 0, nullptr, vrows, &ci, 10, &cfo, &cio); });
  rc |= refused("components lengths", "one entry a sequence",
                [&] { n3::GatherStoredChunkInput(nullptr, -5, 21, 3, 4, vutt, std::vector<int>(1, 0), 0, nullptr, vrows, &ci, 10, &cfo, &cio); });
  // the host-only entries: the layout's 64-bit offsets, a payload packed (transposed, p0..p3 computed), a float matrix compressed
  const int frames[2] = {13, 30};
  long long offsets[3], bytes = 0;
  if (tdnnf_feature_store_layout(1, 5, 2, frames, offsets, &bytes) != TDNNF_OK || offsets[1] != 80 || offsets[2] != 240 || bytes != 240 + 2 * (32 + 80)) rc |= 1;
  float header[12];
  uint8_t packed[6];
  if (tdnnf_feature_store_pack(3, &item, header, packed) != TDNNF_OK || packed[1] != 65 || packed[2] != 193 || packed[3] != 64 || header[0] != -2.f) rc |= 1;
  std::printf("layout and pack: %lld bytes, header[3] %g\n", bytes, header[3]);
  const float x[4] = {1.f, 2.f, 3.f, 5.f};
  float mn = 0, range = 0;
  uint8_t c8[4];
  if (tdnnf_feature_store_compress(3, 2, 2, x, &mn, &range, c8) != TDNNF_OK || mn != 1.f || range != 4.f || c8[0] != 0 || c8[3] != 255) rc |= 1;
  if (tdnnf_feature_store_compress(1, 2, 2, x, &mn, &range, c8) != TDNNF_EINVAL || !std::strstr(tdnnf_last_error(), "format 1 (CM) from float matrices is not built"))
    rc |= 1;
  std::printf("compress: %s\n", tdnnf_last_error());
  if (tdnnf_feature_store_pack(8, &item, header, packed) != TDNNF_EINVAL || !std::strstr(tdnnf_last_error(), "item 0 has 3 columns, feat_dim is 8")) rc |= 1;
  std::printf("pack: %s\n", tdnnf_last_error());
  return rc;
}
