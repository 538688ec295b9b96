// chunk_input_kernels.h -- the device half of the chunk minibatch inputs (include/tdnnf_hip.h, "CHUNK INPUTS"; chunk_input.hip): the
// training-side sibling of infer_gather_kernel (infer.hip).  A grid-stride copy through the table of chunk_input_plan.h: no arithmetic, every
// byte read once and written once.
#pragma once
#include "chunk_input_plan.h"
#include "common.h"

namespace tdnnf {

// out row k B + b (k < num_t) = feature row clamp(tab[b][2] + first_t + k, 0, tab[b][1] - 1) of the utterance that starts at stacked row
// tab[b][0]; behind those elements, iv_out row b = stacked i-vector row tab[b][3] (iv_out.cols 0: none).  Consecutive lanes take
// consecutive columns of one output row, so a wave reads and writes runs of whole rows.  VEC 4: 16-byte loads and stores (every width a
// multiple of 4 floats, every stride and base pointer of 16 bytes: chosen on the host).
template <int VEC>
__global__ __launch_bounds__(256) void chunk_input_gather_kernel(MatView feats, MatView iv, const int *tab, int B, int first_t, MatView out, MatView iv_out) {
  const int cv = out.cols / VEC, icv = iv_out.cols / VEC;
  const long long feat_total = (long long)out.rows * cv, total = feat_total + (long long)B * icv;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const float *src;
    float *dst;
    if (e < feat_total) {
      const int r = (int)(e / cv), c = (int)(e % cv) * VEC, k = r / B, b = r % B;
      const int *ch = tab + kChunkTab * b;
      const long long at = (long long)ch[2] + first_t + k;
      const int t = at < 0 ? 0 : (at >= ch[1] ? ch[1] - 1 : (int)at);
      src = feats.data + (size_t)(ch[0] + t) * feats.stride + c;
      dst = out.data + (size_t)r * out.stride + c;
    } else {
      const long long i = e - feat_total;
      const int b = (int)(i / icv), c = (int)(i % icv) * VEC;
      src = iv.data + (size_t)tab[kChunkTab * b + 3] * iv.stride + c;
      dst = iv_out.data + (size_t)b * iv_out.stride + c;
    }
    if (VEC == 4) *reinterpret_cast<float4 *>(dst) = *reinterpret_cast<const float4 *>(src);
    else *dst = *src;
  }
}

}  // namespace tdnnf
