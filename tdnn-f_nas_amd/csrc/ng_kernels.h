// ng_kernels.h -- the small device kernels of ng_stats.hip: what it launches around the N-sized passes (stack_taps_kernel,
// pform_combine_kernel, scatter_col_kernel, ng_scalars_kernel) and the two ends of the per-object chain (set_column_kernel,
// ng_commit_kernel).  The N-sized work itself is the rows GEMM / weight gradient of gemm_f32.h and ng_valu.hip; the grouped chain's
// kernels are in ng_group_kernels.h.  Included into ng_stats.hip's anonymous namespace and nowhere else: every unit that includes it
// adds a copy of each kernel to the library, launched or not -- which is why the two kernels of the refresh sit in ng_refresh.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "gemm_f32.h"

namespace tdnnf {
namespace {

// ------------------------------------------------------------------ statistics passes (ng_stats.hip)
// WP[(i * Rp + r) * Di + k] = W[r * Dp + i * Di + k]: the taps' blocks of W_t one below the other (K Rp x Di, k contiguous)
__global__ void stack_taps_kernel(const float *W, int Rp, int Dp, int Di, int K, float *WP) {
  const long long total = (long long)K * Rp * Di;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int k = (int)(e % Di), ir = (int)(e / Di), i = ir / Rp, r = ir % Rp;
    WP[e] = W[(size_t)r * Dp + (size_t)i * Di + k];
  }
}
// H[m][r] = sum_i P[m + o_i][i * Rp + r] (+ bias[r]);  part[b] = sum_i psum[b + o_i / 128] for the 128-row block b (o_i % 128 == 0)
struct PformTaps {
  int K, o[kMaxSeg];
};
__global__ __launch_bounds__(256) void pform_combine_kernel(const float *P, int ldp, PformTaps tp, int Rp, const float *bias, float *H, int N,
                                                            const double *psum, double *part, int part_cap) {
  const int m0 = blockIdx.x * 128, per = Rp / 4;  // float4 per row of H
  for (int e = threadIdx.x; e < 128 * per; e += 256) {
    const int m = m0 + e / per, q = e % per;
    if (m >= N) break;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (bias) v = *reinterpret_cast<const float4 *>(bias + 4 * q);
    for (int i = 0; i < tp.K; i++) {
      const float4 t = *reinterpret_cast<const float4 *>(P + (size_t)(m + tp.o[i]) * ldp + i * Rp + 4 * q);
      v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
    }
    *reinterpret_cast<float4 *>(H + (size_t)m * Rp + 4 * q) = v;
  }
  if (threadIdx.x == 0) {
    double sacc = 0;
    for (int i = 0; i < tp.K; i++) sacc += psum[blockIdx.x + tp.o[i] / 128];
    part[blockIdx.x] = sacc;
  }
  for (int i = gridDim.x + blockIdx.x * 256 + threadIdx.x; i < part_cap; i += gridDim.x * 256) part[i] = 0.0;
}
__global__ void scatter_col_kernel(const float *v, int R, float *J, int ld, int col) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < R) J[(size_t)r * ld + col] = v[r];
}
// tr0 = sum partial + ones_term;  tr1 = tr0 - 2 tr(L) + <L, WWT>;  scale = sqrt(tr0 / tr1)
__global__ __launch_bounds__(256) void ng_scalars_kernel(const double *partial, int nb, double ones_term, const float *L, const float *WWT,
                                                         int Rp, double *scal, float *scale_f) {
  __shared__ double red[3][4];
  double a = 0, b = 0, c = 0;
  for (int i = threadIdx.x; i < nb; i += 256) a += partial[i];
  for (int i = threadIdx.x; i < Rp * Rp; i += 256) {
    const double l = L[i];
    c += l * (double)WWT[i];
    if (i / Rp == i % Rp) b += l;
  }
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
    c += __shfl_xor(c, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = a;
    red[1][threadIdx.x >> 6] = b;
    red[2][threadIdx.x >> 6] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double tr0 = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]) + ones_term;
    const double trL = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    const double trLW = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
    const double tr1 = tr0 - 2.0 * trL + trLW;
    scal[0] = tr0;
    scal[1] = tr1;
    *scale_f = (tr0 <= 0.0 || !(tr1 > 0.0)) ? 1.0f : (float)sqrt(tr0 / tr1);
  }
}

// ------------------------------------------------------------------ per-object chain (ng_stats.hip: ng_set_column, ng_chain_one)
__global__ void set_column_kernel(const float *v, int rows, float *T, int ldT, int col) {  // (and zeros in the row's padding)
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < rows) {
    T[(size_t)r * ldT + col] = v[r];
    for (int c = col + 1; c < ldT; c++) T[(size_t)r * ldT + c] = 0.f;
  }
}
// W_acc[o][c] += a b T[o][c] (c < ldw), bias_acc[o] += a b T[o][ldw]: "local_lrate = scale * learning_rate_"
// (nnet-tdnn-component.cc:604-624); a, b are the two preconditioners' scales, still on the device
__global__ void ng_commit_kernel(const float *T, int ldT, int Do, int ldw, const float *sa, const float *sb, float *W_acc, float *bias_acc) {
  const float sc = sa[0] * sb[0];
  const int C = ldw + (bias_acc ? 1 : 0);
  const long long total = (long long)Do * C;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int o = (int)(e / C), c = (int)(e % C);
    const float v = sc * T[(size_t)o * ldT + c];
    if (c < ldw) W_acc[(size_t)o * ldw + c] += v;
    else bias_acc[o] += v;
  }
}

}  // namespace
}  // namespace tdnnf
