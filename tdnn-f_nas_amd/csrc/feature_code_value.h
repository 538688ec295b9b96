// feature_code_value.h -- the value of a code of Kaldi's CompressedMatrix and the code of a value, stated ONCE for the three places that need
// them: the egs reader and writer (egs_io.hip: read_general_matrix, write_matrix), the host half of the feature stores
// (feature_store_plan.h) and the kernels that decode a store (feature_store_kernels.h; include/tdnnf_hip.h, "FEATURE STORES").  Every
// expression is float32 with one rounding an operation, in the order written: the device must not contract a product and a sum into an FMA
// (the pragma), the host build has no FMA target and g++ is not asked for one.  Plain C++ with no device header: the drivers under tests/
// build it with g++.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <limits>

#ifdef __HIP__
#define TDNNF_CODE_FN __host__ __device__ __forceinline__
#else
#define TDNNF_CODE_FN inline
#endif
#ifdef __clang__
#define TDNNF_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define TDNNF_NO_CONTRACT
#endif

namespace tdnnf {

// "CM2" codes, and the four percentiles h0..h3 of a column of "CM": 16 bits over [min, min + range]
TDNNF_CODE_FN float code16_value(float min_value, float range, uint16_t w) {
  TDNNF_NO_CONTRACT
  return min_value + range * (1.0f / 65535.0f) * w;
}

// "CM3" codes: 8 bits over [min, min + range]
TDNNF_CODE_FN float code8_value(float min_value, float range, uint8_t b) {
  TDNNF_NO_CONTRACT
  return min_value + range * (1.0f / 255.0f) * b;
}

// "CM" codes: piecewise linear between the column's percentiles p0..p3 (code16_value of h0..h3), the pieces [0, 64], (64, 192], (192, 255].
// Selects, then one expression: a wave whose lanes hold codes of different pieces does not diverge.
TDNNF_CODE_FN float percentile_code_value(float p0, float p1, float p2, float p3, uint8_t b) {
  TDNNF_NO_CONTRACT
  const bool low = b <= 64, mid = b <= 192;
  const float from = low ? p0 : mid ? p1 : p2, to = low ? p1 : mid ? p2 : p3;
  const int first = low ? 0 : mid ? 64 : 192;
  const float scale = low ? 1.0f / 64.0f : mid ? 1.0f / 128.0f : 1.0f / 63.0f;
  return from + (to - from) * (b - first) * scale;
}

// The writer's rule (kTwoByteAuto, and the same over 8 bits): [min, max] of the matrix, max = min + 1 where not max > min; the code of x
// is (x - min) / range * levels + 0.499 cut to [0, levels], levels = 65535 or 255.
inline void code_range(const float *data, size_t n, float *min_value, float *range) {
  float mn = std::numeric_limits<float>::infinity(), mx = -mn;
  for (size_t i = 0; i < n; i++) {
    mn = std::min(mn, data[i]);
    mx = std::max(mx, data[i]);
  }
  if (!(mx > mn)) mx = mn + 1.0f;
  *min_value = mn;
  *range = mx - mn;
}
inline float value_code(float x, float min_value, float range, float levels) {
  const float f = (x - min_value) / range;
  return std::min(levels, std::max(0.0f, f * levels + 0.499f));
}

}  // namespace tdnnf
