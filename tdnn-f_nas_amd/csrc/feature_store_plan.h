// feature_store_plan.h -- the host half of the feature stores (include/tdnnf_hip.h, "FEATURE STORES"; feature_store.hip): the byte layout of
// a store, the checks of a payload, its packing (header floats, row-major codes) and the compression of a float matrix.  The functions serve
// tdnnf_feature_store_layout / _pack / _compress and the appends alike, so what the host-only entries report is what a store holds.  Plain
// C++ with no device header: tests/feature_store_driver.cc builds it with g++ under the sanitizers.
#pragma once
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <string>

#include "feature_code_value.h"

namespace tdnnf {

// One utterance of a store, as the kernels read it (the store's device table, 32 bytes an utterance).
struct StoreUtt {
  long long code_offset;   // of its first code, in bytes from the store's first: a multiple of 16
  int frames;
  int header_row;          // format 1: its p0..p3 are the float4s [header_row * feat_dim, (header_row + 1) * feat_dim) of the header array
  float min_value, range;  // formats 2 and 3
  int reserved[2];
};
static_assert(sizeof(StoreUtt) == 32, "the table entry is 32 bytes");

// A payload in Kaldi's order, exactly as an archive holds it behind the token.
struct FeaturePayload {
  int format;  // 1 "CM", 2 "CM2", 3 "CM3"
  float min_value, range;
  int rows, cols;
  const uint16_t *percentiles;  // format 1: cols x 4, h0..h3 of every column
  const void *codes;            // format 1: bytes, COLUMN-major (cols x rows); 2: uint16, row-major; 3: bytes, row-major
};

inline bool store_format_ok(int format) { return format >= 1 && format <= 3; }
inline int code_width(int format) { return format == 2 ? 2 : 1; }  // bytes a code
// the bytes an utterance's codes take: every utterance begins at a 16-byte boundary
inline long long utt_code_bytes(int format, int feat_dim, long long frames) { return (frames * feat_dim * code_width(format) + 15) & ~15LL; }
// the bytes behind the codes: the table entry and, in format 1, four floats a column
inline long long utt_side_bytes(int format, int feat_dim) { return (long long)sizeof(StoreUtt) + (format == 1 ? 16LL * feat_dim : 0); }

namespace feature_store_detail {
inline bool refuse(std::string *err, const char *who, const char *fmt, long long a = 0, long long b = 0, long long c = 0) {
  char buf[512], msg[400];
  snprintf(msg, sizeof(msg), fmt, a, b, c);
  snprintf(buf, sizeof(buf), "%s%s", who, msg);
  *err = buf;
  return false;
}
}  // namespace feature_store_detail

// The closed form: code offsets of n utterances appended in this order (offsets: n + 1 entries, the last the codes' total; may be null) and
// the device bytes they take in all.
inline bool feature_store_layout(const char *who, int format, int feat_dim, int n, const int *frames, long long *offsets, long long *device_bytes,
                                 std::string *err) {
  using feature_store_detail::refuse;
  if (!store_format_ok(format)) return refuse(err, who, "format %lld: a store holds format 1 (CM), 2 (CM2) or 3 (CM3)", format);
  if (feat_dim < 1) return refuse(err, who, "feat_dim %lld must be positive", feat_dim);
  if (n < 0 || (n > 0 && !frames)) return refuse(err, who, "%lld utterances need their frames", n);
  long long at = 0, rows = 0;
  for (int u = 0; u < n; u++) {
    if (frames[u] < 1) return refuse(err, who, "utterance %lld has %lld frames", u, frames[u]);
    rows += frames[u];
  }
  if (rows >= (1LL << 31)) return refuse(err, who, "%lld frames in all: a store holds at most 2^31 - 1", rows);
  for (int u = 0; u < n; u++) {
    if (offsets) offsets[u] = at;
    at += utt_code_bytes(format, feat_dim, frames[u]);
  }
  if (offsets) offsets[n] = at;
  if (device_bytes) *device_bytes = at + n * utt_side_bytes(format, feat_dim);
  return true;
}

// The checks of one payload against a store's format and feat_dim; `index` names it in the message.
inline bool feature_payload_check(const char *who, int index, int format, int feat_dim, const FeaturePayload &p, std::string *err) {
  using feature_store_detail::refuse;
  if (p.format != format) return refuse(err, who, "item %lld is a payload of format %lld, the store holds format %lld", index, p.format, format);
  if (p.cols != feat_dim) return refuse(err, who, "item %lld has %lld columns, feat_dim is %lld", index, p.cols, feat_dim);
  if (p.rows < 1) return refuse(err, who, "item %lld has %lld rows", index, p.rows);
  if (!std::isfinite(p.min_value) || !std::isfinite(p.range)) return refuse(err, who, "item %lld: its min or range is not finite", index);
  if (!p.codes || (format == 1 && !p.percentiles)) return refuse(err, who, "item %lld comes without codes (or, in format 1, without percentiles)", index);
  return true;
}

// Packs a checked payload: header (format 1: 4 * cols floats, p0..p3 of every column; else not written) and codes (rows * cols codes,
// row-major: format 1 transposed).
inline void feature_payload_pack(const FeaturePayload &p, float *header, void *codes) {
  const size_t n = (size_t)p.rows * p.cols;
  if (p.format != 1) {
    memcpy(codes, p.codes, n * code_width(p.format));
    return;
  }
  for (int i = 0; i < 4 * p.cols; i++) header[i] = code16_value(p.min_value, p.range, p.percentiles[i]);
  const uint8_t *src = static_cast<const uint8_t *>(p.codes);
  uint8_t *dst = static_cast<uint8_t *>(codes);
  for (int j = 0; j < p.cols; j++)
    for (int i = 0; i < p.rows; i++) dst[(size_t)i * p.cols + j] = src[(size_t)j * p.rows + i];
}

// The checks of a float matrix to compress and its (min, range): the writer's rule (code_range).
inline bool feature_compress_check(const char *who, int index, int format, int rows, int cols, const float *x, float *min_value, float *range, std::string *err) {
  using feature_store_detail::refuse;
  if (format == 1)
    return refuse(err, who, "format 1 (CM) from float matrices is not built: Kaldi's percentile selection; compress to format 2 or 3, or append CM payloads");
  if (!store_format_ok(format)) return refuse(err, who, "format %lld: float matrices compress to format 2 (CM2) or 3 (CM3)", format);
  if (cols < 1) return refuse(err, who, "item %lld has %lld columns", index, cols);
  if (rows < 1) return refuse(err, who, "item %lld has %lld rows", index, rows);
  if (!x) return refuse(err, who, "item %lld comes without a matrix", index);
  code_range(x, (size_t)rows * cols, min_value, range);
  if (!std::isfinite(*min_value) || !std::isfinite(*range)) return refuse(err, who, "item %lld: its min or range is not finite", index);
  return true;
}

// The codes of a checked float matrix: uint16 (format 2) or bytes (format 3), row-major.
inline void feature_compress(int format, int rows, int cols, const float *x, float min_value, float range, void *codes) {
  const size_t n = (size_t)rows * cols;
  if (format == 2) {
    uint16_t *w = static_cast<uint16_t *>(codes);
    for (size_t i = 0; i < n; i++) w[i] = (uint16_t)value_code(x[i], min_value, range, 65535.0f);
  } else {
    uint8_t *b = static_cast<uint8_t *>(codes);
    for (size_t i = 0; i < n; i++) b[i] = (uint8_t)value_code(x[i], min_value, range, 255.0f);
  }
}

}  // namespace tdnnf
