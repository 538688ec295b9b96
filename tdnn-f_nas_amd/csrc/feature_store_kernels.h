// feature_store_kernels.h -- the device half of the feature stores (include/tdnnf_hip.h, "FEATURE STORES"; feature_store.hip): the two
// kernels that decode a store's codes while they copy.  feature_store_gather_kernel is chunk_input_gather_kernel (chunk_input_kernels.h)
// with the source row decoded -- the same grid-stride walk over output elements, the same table, the i-vector rows in the same launch --,
// feature_store_expand_kernel the same loop over (entry of a list of utterances, row, column).  The values are those of
// feature_code_value.h, float32, one rounding an operation, never contracted.  VEC 4: a lane takes 4 columns -- its 4 codes in one 4-byte
// load (formats 1, 3) or one 8-byte load (format 2), in format 1 its columns' p0..p3 as four float4s (16 x feat_dim bytes an utterance,
// read by every row of it: resident in L2), one 16-byte store; chosen on the host where feat_dim is a multiple of 4 and the output's
// stride and base pointer allow 16 bytes (inside the store every utterance begins at a 16-byte boundary, so row r column c of a feat_dim
// that is a multiple of 4 is 4 codes from a 4-code boundary).  VEC 1: a code at a time; in format 1 it still reads its column's whole
// float4 of percentiles for the one code (16 bytes out of L2 a value written, of which two floats are used): the slow tail of a feat_dim
// that is no multiple of 4, not measured.  No LDS, no atomics, no scratch; every store a
// plain vector store.  gfx950, VGPRs (accumulation registers 0, scratch 0, LDS 0 in every form):
//   gather  format 1 / 2 / 3, VEC 4: 39 / 18 / 17    VEC 1: 28 / 20 / 20
//   expand  format 1 / 2 / 3, VEC 4: 35 / 18 / 16    VEC 1: 22 / 18 / 16
// and no FMA in any decode (the v_fmac of the listings belong to the 64-bit division of the element index).
#pragma once
#include "chunk_input_plan.h"
#include "common.h"
#include "feature_store_plan.h"

namespace tdnnf {

struct StoreView {
  const unsigned char *codes;  // every utterance's codes, row-major, at StoreUtt::code_offset
  const float4 *headers;       // format 1: p0..p3 of column j of the utterance at [header_row * feat_dim + j]
  const StoreUtt *utts;
  int feat_dim;
};

// Decodes columns [c, c + VEC) of row t of utterance su into dst.
template <int FMT, int VEC>
__device__ __forceinline__ void store_decode(const StoreView &st, const StoreUtt &su, int t, int c, float *dst) {
  const size_t at = (size_t)t * st.feat_dim + c;  // in codes, from the utterance's first
  float v[VEC];
  if constexpr (FMT == 2) {
    const uint16_t *p = reinterpret_cast<const uint16_t *>(st.codes + su.code_offset) + at;
    if constexpr (VEC == 4) {
      const uint2 w = *reinterpret_cast<const uint2 *>(p);
      v[0] = code16_value(su.min_value, su.range, (uint16_t)(w.x & 0xffffu));
      v[1] = code16_value(su.min_value, su.range, (uint16_t)(w.x >> 16));
      v[2] = code16_value(su.min_value, su.range, (uint16_t)(w.y & 0xffffu));
      v[3] = code16_value(su.min_value, su.range, (uint16_t)(w.y >> 16));
    } else {
      v[0] = code16_value(su.min_value, su.range, *p);
    }
  } else {
    const unsigned char *p = st.codes + su.code_offset + at;
    const unsigned w = VEC == 4 ? *reinterpret_cast<const unsigned *>(p) : *p;
#pragma unroll
    for (int i = 0; i < VEC; i++) {
      const uint8_t b = (uint8_t)((w >> (8 * i)) & 0xffu);
      if constexpr (FMT == 1) {
        const float4 q = st.headers[(size_t)su.header_row * st.feat_dim + c + i];
        v[i] = percentile_code_value(q.x, q.y, q.z, q.w, b);
      } else {
        v[i] = code8_value(su.min_value, su.range, b);
      }
    }
  }
  if constexpr (VEC == 4) *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
  else *dst = v[0];
}

// out row k B + b (k < num_t) = the decoded row clamp(tab[b][2] + first_t + k, 0, tab[b][1] - 1) of the store's utterance tab[b][0]; behind
// those elements, iv_out row b = stacked i-vector row tab[b][3] (iv_out.cols 0: none), floats as in chunk_input_gather_kernel.
template <int FMT, int VEC>
__global__ __launch_bounds__(256) void feature_store_gather_kernel(StoreView st, MatView iv, const int *tab, int B, int first_t, MatView out, MatView iv_out) {
  const int cv = out.cols / VEC, icv = iv_out.cols / VEC;
  const long long feat_total = (long long)out.rows * cv, total = feat_total + (long long)B * icv;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    if (e < feat_total) {
      const int r = (int)(e / cv), c = (int)(e % cv) * VEC, k = r / B, b = r % B;
      const int *ch = tab + kChunkTab * b;
      const long long at = (long long)ch[2] + first_t + k;
      const int t = at < 0 ? 0 : (at >= ch[1] ? ch[1] - 1 : (int)at);
      store_decode<FMT, VEC>(st, st.utts[ch[0]], t, c, out.data + (size_t)r * out.stride + c);
    } else {
      const long long i = e - feat_total;
      const int b = (int)(i / icv), c = (int)(i % icv) * VEC;
      const float *src = iv.data + (size_t)tab[kChunkTab * b + 3] * iv.stride + c;
      float *dst = iv_out.data + (size_t)b * iv_out.stride + c;
      if (VEC == 4) *reinterpret_cast<float4 *>(dst) = *reinterpret_cast<const float4 *>(src);
      else *dst = *src;
    }
  }
}

// out row list[i][1] + t = the decoded row t of the store's utterance list[i][0], t < its frames, i < n: list[i][1] is the first output row
// of entry i (ascending, list[0][1] = 0), rows their total.  The entry of a row is found by bisection of those n first rows.
template <int FMT, int VEC>
__global__ __launch_bounds__(256) void feature_store_expand_kernel(StoreView st, const int *list, int n, MatView out) {
  const int cv = out.cols / VEC;
  const long long total = (long long)out.rows * cv;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int r = (int)(e / cv), c = (int)(e % cv) * VEC;
    int lo = 0, hi = n - 1;  // the last entry whose first row is <= r
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (list[2 * mid + 1] <= r) lo = mid;
      else hi = mid - 1;
    }
    store_decode<FMT, VEC>(st, st.utts[list[2 * lo]], r - list[2 * lo + 1], c, out.data + (size_t)r * out.stride + c);
  }
}

}  // namespace tdnnf
