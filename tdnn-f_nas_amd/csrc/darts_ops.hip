// darts_ops.hip -- the DARTS mixing components: (Gumbel)Softmax(Flops), Onehot, CopyN, ConstantFunction, FlopsConstraint,
// ElementwiseProduct, and the mixing coefficients of a TDNN component's taps with their update (darts_coef, alpha_update).  Small
// matrices (8 columns in every recipe): one kernel per component pass, grid-stride, grids capped at 2048 blocks.
//
// Reference: /root/reference/src/nnet3/nnet-simple-component.cc, nnet-tdnn-component.cc (exact line ranges are next to each C-ABI
// entry in include/tdnnf_hip.h).
#include <algorithm>

#include "colreduce.h"
#include "ew_dev.h"

namespace tdnnf {
namespace {

// one thread per row; the row stays in `out` between the passes (C is 8 in every recipe)
__global__ void softmax_rows_kernel(MatView in, const float *gumbel_u, float inv_temp, MatView out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= in.rows) return;
  const float *x = in.data + (long long)r * in.stride;
  float *o = out.data + (long long)r * out.stride;
  for (int c = 0; c < in.cols; c++) o[c] = gumbel_u ? (x[c] + gumbel(gumbel_u[c])) * inv_temp : x[c];
  softmax_short_row(o, in.cols);
}
__global__ void softmax_flops_bwd_kernel(MatView p, MatView dp, float a, const float *flops, int dim, float inv_temp,
                                         MatView dx) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= p.rows) return;
  const float *pv = p.data + (long long)r * p.stride;
  float *e = dp.data + (long long)r * dp.stride;
  float *d = dx.data + (long long)r * dx.stride;
  if (flops)
    for (int c = 0; c < dim; c++) e[c] += a * flops[c];
  float pe = 0.f;
  for (int c = 0; c < p.cols; c++) pe += pv[c] * e[c];
  for (int c = 0; c < p.cols; c++) d[c] = pv[c] * (e[c] - pe) * inv_temp;
}
__global__ void onehot_kernel(const float *u, MatView out) {
  const float uu = u[0];
  const int C = out.cols;
  const long long total = (long long)out.rows * C;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int r = (int)(e / C), c = (int)(e % C);
    out.data[(long long)r * out.stride + c] = onehot_bucket(uu, c, C);
  }
}
__global__ void copyn_fwd_kernel(MatView in, float scale, MatView out) {
  const int C = out.cols, d = in.cols;
  const long long total = (long long)out.rows * C;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int r = (int)(e / C), c = (int)(e % C);
    out.data[(long long)r * out.stride + c] += scale * in.data[(long long)r * in.stride + c % d];
  }
}
__global__ void copyn_bwd_kernel(MatView dout, float scale, MatView din) {
  const int d = din.cols, nb = dout.cols / d;
  const long long total = (long long)din.rows * d;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int r = (int)(e / d), c = (int)(e % d);
    float s = 0.f;
    for (int b = 0; b < nb; b++) s += dout.data[(long long)r * dout.stride + b * d + c];
    din.data[(long long)r * din.stride + c] += scale * s;
  }
}
__global__ void rows_from_vec_kernel(const float *v, float scale, MatView out) {
  const int C = out.cols;
  const long long total = (long long)out.rows * C;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL)
    out.data[(e / C) * out.stride + e % C] = scale * v[e % C];
}
__global__ void ewprod_fwd_kernel(MatView in, int od, MatView out) {
  const int n = in.cols / od;
  const long long total = (long long)in.rows * od;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int r = (int)(e / od), c = (int)(e % od);
    const float *x = in.data + (long long)r * in.stride;
    float p = x[c];
    for (int i = 1; i < n; i++) p *= x[i * od + c];
    out.data[(long long)r * out.stride + c] = p;
  }
}
__global__ void ewprod_bwd_kernel(MatView in, MatView dout, int od, MatView din) {
  const int n = in.cols / od;
  const long long total = (long long)in.rows * in.cols;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int r = (int)(e / in.cols), cc = (int)(e % in.cols), i = cc / od, c = cc % od;
    const float *x = in.data + (long long)r * in.stride;
    float p = dout.data[(long long)r * dout.stride + c];
    for (int j = 0; j < n; j++)
      if (j != i) p *= x[j * od + c];
    din.data[(long long)r * din.stride + cc] = p;
  }
}

// One wave; K <= 16.  Restates nnet-tdnn-component.cc:250-289 and the effective weights of :292-328.
__global__ void darts_coef_kernel(const float *log_alpha, int K, int flags, float temp, const float *gu,
                                  const float *su, int share, float *coef, float *eff) {
  if (threadIdx.x != 0) return;
  float c[TDNNF_MAX_OFFSETS];
  for (int i = 0; i < K; i++) c[i] = log_alpha[i];
  if (flags & TDNNF_DARTS_USE_GUMBEL) {
    for (int i = 0; i < K; i++) c[i] = (c[i] + gumbel(gu[i])) * (1.0f / temp);
  }
  if ((flags & TDNNF_DARTS_USE_GUMBEL) || !(flags & TDNNF_DARTS_FREE_SELECT)) {
    softmax_short_row(c, K);
  } else {
    for (int i = 0; i < K; i++) c[i] = 1.0f / (1.0f + expf(-c[i]));
  }
  if (flags & TDNNF_DARTS_UNIFORM_SAMPLE) {
    const float u = su[0];
    for (int i = 0; i < K; i++) c[i] = onehot_bucket(u, i, K);
  }
  for (int i = 0; i < K; i++) {
    coef[i] = c[i];
    float e;
    if (flags & TDNNF_DARTS_UNIFORM_SAMPLE) e = (i == share || c[i] == 1.f) ? 1.f : 0.f;
    else if (flags & TDNNF_DARTS_FREE_SELECT) e = c[i];
    else e = (i == share) ? 1.f : c[i];
    eff[i] = e;
  }
}

// s_i = <dW_i, W_i> per tap, two-stage and ordered: block (tap, slab) reduces a slab of output rows into partial[tap][slab]
// (float4 reads, no index arithmetic per element), alpha_update_kernel adds a tap's slabs in slab order.
// dots: [K | K * TDNNF_TAP_DOTS_SLABS] doubles (s_i, then the partials).
__global__ __launch_bounds__(256) void tap_dots_kernel(const float *G, int ldg, const float *W, int ldw, int Do, int Di, int K, int vec,
                                                       double *dots) {
  __shared__ double red[4];
  const int tap = blockIdx.x, slab = blockIdx.y, nslab = gridDim.y;
  const int rows = (Do + nslab - 1) / nslab, o0 = slab * rows, o1 = min(Do, o0 + rows);
  double s = 0;
  if (vec) {  // Di, both leading dimensions and both pointers allow 16-byte reads
    const int q = Di >> 2;
    for (int e = threadIdx.x; e < (o1 - o0) * q; e += 256) {
      const int o = o0 + e / q, d = (e % q) << 2;
      const float4 g = *reinterpret_cast<const float4 *>(G + (long long)o * ldg + tap * Di + d);
      const float4 w = *reinterpret_cast<const float4 *>(W + (long long)o * ldw + tap * Di + d);
      s += ((double)g.x * (double)w.x + (double)g.y * (double)w.y) + ((double)g.z * (double)w.z + (double)g.w * (double)w.w);
    }
  } else {
    for (int e = threadIdx.x; e < (o1 - o0) * Di; e += 256) {
      const int o = o0 + e / Di, d = e % Di;
      s += (double)G[(long long)o * ldg + tap * Di + d] * (double)W[(long long)o * ldw + tap * Di + d];
    }
  }
  s = block_sum256(s, red);
  if (threadIdx.x == 0) dots[K + tap * nslab + slab] = s;
}
__global__ void alpha_update_kernel(double *dots, int nslab, const float *coef, int K, int flags, int share, float temp,
                                    float lr, float *acc) {
  // the slabs of a tap: one per lane, then a fixed shuffle tree (one wave; nslab <= 64) -- a serial chain of K x 64 dependent loads took 65 us
  if (nslab > 0) {
    for (int i = 0; i < K; i++) {
      const double s = wave_sum((int)threadIdx.x < nslab ? dots[K + i * nslab + threadIdx.x] : 0.0);
      if (threadIdx.x == 0) dots[i] = s;
    }
  }
  if (threadIdx.x != 0) return;
  if (!(flags & TDNNF_DARTS_UNIFORM_SAMPLE)) {
    for (int i = 0; i < K; i++) {
      const float si = (float)dots[i];
      if (flags & TDNNF_DARTS_FREE_SELECT) {
        acc[i] += si * coef[i];
        acc[i] += -1.0f * si * coef[i] * coef[i];
      } else if (i != share) {
        const float tau = (flags & TDNNF_DARTS_USE_GUMBEL) ? temp : 1.0f;
        for (int j = 0; j < K; j++) acc[j] += (-1.0f * si / tau) * coef[i] * coef[j];
        acc[i] += (si / tau) * coef[i];
      }
    }
  }
  float mul = 1.0f;
  if (flags & TDNNF_DARTS_USE_ENTROPY) mul *= 5.0f;
  if (flags & TDNNF_DARTS_FREE_SELECT) mul *= 5.0f * lr;
  else if (flags & TDNNF_DARTS_USE_GUMBEL) mul *= lr;
  else mul *= 5.0f * lr;
  if (flags & TDNNF_DARTS_UPDATE_ALPHA) mul *= 10000.0f;
  for (int i = 0; i < K; i++) acc[i] *= mul;
}

}  // namespace
}  // namespace tdnnf

using namespace tdnnf;

extern "C" {

int tdnnf_softmax_flops_propagate(const tdnnf_mat *in, const float *gumbel_u, float temp, tdnnf_mat *out, tdnnf_stream stream) {
  TDNNF_REQUIRE(mat_ok(in) && mat_ok(out) && same_dim(in, out) && in->cols > 0, "softmax_flops_propagate: bad matrices");
  TDNNF_REQUIRE(!gumbel_u || temp > 0, "softmax_flops_propagate: temp-proportion must be > 0");
  if (in->rows == 0) return TDNNF_OK;
  hipLaunchKernelGGL(softmax_rows_kernel, dim3((in->rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, view(in), gumbel_u,
                     gumbel_u ? 1.0f / temp : 1.0f, view(out));
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

int tdnnf_softmax_flops_backprop(const tdnnf_mat *out_value, tdnnf_mat *out_deriv, float scale, const float *flops, int dim,
                                 float temp, tdnnf_mat *in_deriv, tdnnf_stream stream) {
  TDNNF_REQUIRE(mat_ok(out_value) && mat_ok(out_deriv) && mat_ok(in_deriv) && same_dim(out_value, out_deriv) &&
                    same_dim(out_value, in_deriv),
                "softmax_flops_backprop: bad matrices");
  TDNNF_REQUIRE(temp > 0 && (!flops || (dim > 0 && dim <= out_value->cols)), "softmax_flops_backprop: bad temp/dim");
  if (out_value->rows == 0) return TDNNF_OK;
  const float a = scale / out_deriv->rows / out_deriv->cols;
  hipLaunchKernelGGL(softmax_flops_bwd_kernel, dim3((out_value->rows + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     view(out_value), view(out_deriv), a, flops, dim, 1.0f / temp, view(in_deriv));
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

int tdnnf_onehot_propagate(const float *u, tdnnf_mat *out, tdnnf_stream stream) {
  TDNNF_REQUIRE(u && mat_ok(out), "onehot_propagate: bad arguments");
  if (out->rows * out->cols == 0) return TDNNF_OK;
  hipLaunchKernelGGL(onehot_kernel, dim3(grid_for((long long)out->rows * out->cols, 256)), dim3(256), 0, (hipStream_t)stream, u, view(out));
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

int tdnnf_copyn_propagate(const tdnnf_mat *in, float scale, tdnnf_mat *out, tdnnf_stream stream) {
  TDNNF_REQUIRE(mat_ok(in) && mat_ok(out) && in->rows == out->rows && in->cols > 0 && out->cols % in->cols == 0,
                "copyn_propagate: output-dim must be a multiple of input-dim");
  if (out->rows == 0) return TDNNF_OK;
  hipLaunchKernelGGL(copyn_fwd_kernel, dim3(grid_for((long long)out->rows * out->cols, 256)), dim3(256), 0, (hipStream_t)stream, view(in), scale, view(out));
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}
int tdnnf_copyn_backprop(const tdnnf_mat *out_deriv, float scale, tdnnf_mat *in_deriv, tdnnf_stream stream) {
  TDNNF_REQUIRE(mat_ok(out_deriv) && mat_ok(in_deriv) && in_deriv->rows == out_deriv->rows && in_deriv->cols > 0 &&
                    out_deriv->cols % in_deriv->cols == 0,
                "copyn_backprop: output-dim must be a multiple of input-dim");
  if (in_deriv->rows == 0) return TDNNF_OK;
  hipLaunchKernelGGL(copyn_bwd_kernel, dim3(grid_for((long long)in_deriv->rows * in_deriv->cols, 256)), dim3(256), 0, (hipStream_t)stream, view(out_deriv), scale, view(in_deriv));
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

int tdnnf_constant_function_propagate(const float *output, tdnnf_mat *out, tdnnf_stream stream) {
  TDNNF_REQUIRE(output && mat_ok(out), "constant_function_propagate: bad arguments");
  if (out->rows * out->cols == 0) return TDNNF_OK;
  hipLaunchKernelGGL(rows_from_vec_kernel, dim3(grid_for((long long)out->rows * out->cols, 256)), dim3(256), 0, (hipStream_t)stream, output, 1.0f, view(out));
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}
// ConstantFunctionComponent, non-NG branch: output += 5 lr colsum(out_deriv) (the one-hot component below takes lr itself)
int tdnnf_constant_function_backprop(const tdnnf_mat *out_deriv, float lr, float *output_acc, void *ws, size_t ws_bytes,
                                     tdnnf_stream stream) {
  TDNNF_REQUIRE(mat_ok(out_deriv) && output_acc, "constant_function_backprop: bad arguments");
  if (out_deriv->rows == 0) return TDNNF_OK;
  TDNNF_REQUIRE(ws && ws_bytes >= colreduce_bytes(out_deriv->rows, out_deriv->cols), "constant_function_backprop: workspace too small");
  TDNNF_HIP(colsum_add(view(out_deriv), 5.0f * lr, output_acc, ws, (hipStream_t)stream));
  return TDNNF_OK;
}

// OnehotFunctionComponent::Backprop nnet-simple-component.cc:9521-9552, the branch the recipes configure
// ("is-updatable=true use-natural-gradient=false", generate_bottleneckCB8share_onehottrain_config.py:12):
// output_.AddRowSumMat(learning_rate, out_deriv); the component has no input derivative
int tdnnf_onehot_backprop(const tdnnf_mat *out_deriv, float lr, float *output_acc, void *ws, size_t ws_bytes, tdnnf_stream stream) {
  TDNNF_REQUIRE(mat_ok(out_deriv) && output_acc, "onehot_backprop: bad arguments");
  if (out_deriv->rows == 0) return TDNNF_OK;
  TDNNF_REQUIRE(ws && ws_bytes >= colreduce_bytes(out_deriv->rows, out_deriv->cols), "onehot_backprop: workspace too small");
  TDNNF_HIP(colsum_add(view(out_deriv), lr, output_acc, ws, (hipStream_t)stream));
  return TDNNF_OK;
}

int tdnnf_flops_constraint_backprop(const float *flops, float scale, int rows_in, int cols_in, tdnnf_mat *in_deriv, tdnnf_stream stream) {
  TDNNF_REQUIRE(flops && mat_ok(in_deriv) && rows_in > 0 && cols_in > 0, "flops_constraint_backprop: bad arguments");
  if (in_deriv->rows * in_deriv->cols == 0) return TDNNF_OK;
  hipLaunchKernelGGL(rows_from_vec_kernel, dim3(grid_for((long long)in_deriv->rows * in_deriv->cols, 256)), dim3(256), 0,
                     (hipStream_t)stream, flops, scale / rows_in / cols_in, view(in_deriv));
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

int tdnnf_elementwise_product_propagate(const tdnnf_mat *in, int output_dim, tdnnf_mat *out, tdnnf_stream stream) {
  TDNNF_REQUIRE(mat_ok(in) && mat_ok(out) && output_dim > 0 && in->cols > output_dim && in->cols % output_dim == 0 &&
                    out->cols == output_dim && out->rows == in->rows,
                "elementwise_product_propagate: input-dim must be a proper multiple of output-dim");
  if (in->rows == 0) return TDNNF_OK;
  hipLaunchKernelGGL(ewprod_fwd_kernel, dim3(grid_for((long long)in->rows * output_dim, 256)), dim3(256), 0, (hipStream_t)stream, view(in), output_dim, view(out));
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}
int tdnnf_elementwise_product_backprop(const tdnnf_mat *in_value, const tdnnf_mat *out_deriv, int output_dim,
                                       tdnnf_mat *in_deriv, tdnnf_stream stream) {
  TDNNF_REQUIRE(mat_ok(in_value) && mat_ok(out_deriv) && mat_ok(in_deriv) && same_dim(in_value, in_deriv) && output_dim > 0 &&
                    in_value->cols % output_dim == 0 && out_deriv->cols == output_dim && out_deriv->rows == in_value->rows,
                "elementwise_product_backprop: bad dimensions");
  if (in_value->rows == 0) return TDNNF_OK;
  hipLaunchKernelGGL(ewprod_bwd_kernel, dim3(grid_for((long long)in_value->rows * in_value->cols, 256)), dim3(256), 0, (hipStream_t)stream, view(in_value), view(out_deriv), output_dim, view(in_deriv));
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

int tdnnf_tdnn_darts_coef(const float *log_alpha, int K, int flags, float temp, const float *gumbel_u, const float *sample_u,
                          int share_index, float *coef_memo, float *eff_coef, tdnnf_stream stream) {
  TDNNF_REQUIRE(log_alpha && coef_memo && eff_coef && K >= 1 && K <= TDNNF_MAX_OFFSETS, "tdnn_darts_coef: K out of range");
  TDNNF_REQUIRE(!(flags & TDNNF_DARTS_USE_GUMBEL) || (gumbel_u && temp > 0), "tdnn_darts_coef: gumbel mode needs draws and temp > 0");
  TDNNF_REQUIRE(!(flags & TDNNF_DARTS_UNIFORM_SAMPLE) || sample_u, "tdnn_darts_coef: uniform-sample mode needs a draw");
  TDNNF_REQUIRE(share_index >= 0 && share_index < K, "tdnn_darts_coef: bad share index");
  hipLaunchKernelGGL(darts_coef_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, log_alpha, K, flags, temp, gumbel_u, sample_u, share_index, coef_memo, eff_coef);
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

int tdnnf_tdnn_darts_alpha_update(const float *tap_grad, int ldg, const float *W, int ldw, int Do, int Di, int K,
                                  const float *coef_memo, int flags, int share_index, float temp, float lr,
                                  float *alpha_acc, double *tap_dots, tdnnf_stream stream) {
  // uniform-sample mode adds no gradient (the reference computes and discards it, :502-507): only the scalings run and
  // tap_grad may be null
  const bool uniform = (flags & TDNNF_DARTS_UNIFORM_SAMPLE) != 0;
  TDNNF_REQUIRE((tap_grad || uniform) && W && coef_memo && alpha_acc && tap_dots, "tdnn_darts_alpha_update: null pointer (tap_dots_dev is required scratch of TDNNF_TAP_DOTS_DOUBLES(K) doubles)");
  TDNNF_REQUIRE(K >= 1 && K <= TDNNF_MAX_OFFSETS && Do > 0 && Di > 0 && ldg >= K * Di && ldw >= K * Di, "tdnn_darts_alpha_update: bad dimensions");
  const int nslab = std::min(TDNNF_TAP_DOTS_SLABS, Do);
  if (tap_grad) {
    const int vec = Di % 4 == 0 && ldg % 4 == 0 && ldw % 4 == 0 && ((reinterpret_cast<uintptr_t>(tap_grad) | reinterpret_cast<uintptr_t>(W)) & 15) == 0;
    hipLaunchKernelGGL(tap_dots_kernel, dim3(K, nslab), dim3(256), 0, (hipStream_t)stream, tap_grad, ldg, W, ldw, Do, Di, K, vec, tap_dots);
  }
  hipLaunchKernelGGL(alpha_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, tap_dots, tap_grad ? nslab : 0, coef_memo, K, flags, share_index, temp, lr, alpha_acc);
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

}  // extern "C"
