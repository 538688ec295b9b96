// elementwise.hip -- HBM-bound maps for gfx950: ReLU (with its statistics and self-repair), scaled sums, dropout, and the dot / axpy of
// two parameter vectors.  One kernel replaces each chain of CuMatrix calls of the reference; loads and stores are 16 B
// per lane when the views allow it; the maps are grid-stride with grids capped at 2048 blocks.  The column reduction, BatchNorm,
// LogSoftmax and the DARTS mixing ops are colreduce.hip, batchnorm.hip, log_softmax.hip and darts_ops.hip.
//
// Reference: /root/reference/src/nnet3/nnet-simple-component.cc
// (exact line ranges are next to each C-ABI entry in include/tdnnf_hip.h).
#include "colreduce.h"
#include "ew_dev.h"

namespace tdnnf {
namespace {

// OP 0: out = max(a,0)              (relu fwd)
// OP 1: out = (a>0) * b             (relu bwd: a = out_value, b = out_deriv)
// OP 2: out = sa*a + sb*b           (sum of scaled; b may alias out)
// OP 3: out = sa*a                  (scaled copy)
// OP 4: out += sa*a
template <int OP, int VEC>
__global__ __launch_bounds__(256) void ew_kernel(MatView a, MatView b, float sa, float sb, MatView out) {
  const int cv = out.cols / VEC;
  const long long total = (long long)out.rows * cv;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int r = (int)(e / cv), c = (int)(e % cv) * VEC;
    float x[4], y[4], o[4];
    ld(a.data + (long long)r * a.stride + c, x, VEC == 4);
    if (OP == 1 || OP == 2) ld(b.data + (long long)r * b.stride + c, y, VEC == 4);
    if (OP == 4) ld(out.data + (long long)r * out.stride + c, y, VEC == 4);
#pragma unroll
    for (int j = 0; j < VEC; j++) {
      if (OP == 0) o[j] = x[j] < 0.f ? 0.f : x[j];
      if (OP == 1) o[j] = (x[j] > 0.f ? 1.f : 0.f) * y[j];
      if (OP == 2) o[j] = fmaf(sa, x[j], sb * y[j]);  // (spelled out: left to the compiler, VEC 4 contracted this way and VEC 1 not at all)
      if (OP == 3) o[j] = sa * x[j];
      if (OP == 4) o[j] = y[j] + sa * x[j];
    }
    st(out.data + (long long)r * out.stride + c, o, VEC == 4);
  }
}

template <int OP>
hipError_t launch_ew(MatView a, MatView b, float sa, float sb, MatView out, hipStream_t s) {
  if (out.rows == 0 || out.cols == 0) return hipSuccess;
  const bool needb = (OP == 1 || OP == 2);
  const bool vec = vec4_ok(a) && vec4_ok(out) && (!needb || vec4_ok(b));
  return launch_vec_or_scalar(vec, out.rows, out.cols, ew_kernel<OP, 4>, ew_kernel<OP, 1>, s, a, b, sa, sb, out);
}

// relu stats finalize: stats = [count, value_sum[D], deriv_sum[D]]
__global__ void relu_stats_finalize_kernel(const float *partial, int chunks, int D, int rows, double *stats) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d == 0) stats[0] += (double)rows;
  if (d >= D) return;
  double vs = 0, ds = 0;
  for (int c = 0; c < chunks; c++) {
    vs += partial[(long long)c * D + d];
    ds += partial[((long long)chunks + c) * D + d];
  }
  stats[1 + d] += vs;
  stats[1 + D + d] += ds;
}
// RepairGradients (nnet-simple-component.cc:1028-1073): add +-scale/0.5 to the columns outside the thresholds
__global__ void relu_repair_kernel(const double *stats, int D, float self_repair_scale, float lower, float upper,
                                   MatView in_deriv) {
  const float count = (float)stats[0];
  if (self_repair_scale == 0.f || count == 0.f) return;
  const float lo = lower * count, hi = upper * count;
  const long long total = (long long)in_deriv.rows * D;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int r = (int)(e / D), c = (int)(e % D);
    const float st = (float)stats[1 + D + c];
    float v = (st - lo > 0.f ? 1.f : 0.f) + (st - hi > 0.f ? 1.f : 0.f) - 1.f;
    v *= -self_repair_scale / 0.5f;
    if (v != 0.f) in_deriv.data[(long long)r * in_deriv.stride + c] += v;
  }
}

// GeneralDropoutComponent::GetMemo (UPSTREAM): continuous: 1 - 2p + 4p U; else (U - p > 0 ? 1 : 0) / (1 - p)
__global__ void general_dropout_mask_kernel(const float *u, long long n, float p, int continuous, float *mask) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += gridDim.x * 256LL) {
    const float v = u[i];
    mask[i] = continuous ? v * (p * 4.0f) + (1.0f - 2.0f * p) : ((v + -p > 0.0f) ? 1.0f : 0.0f) * (1.0f / (1.0f - p));
  }
}
__global__ void dropout_kernel(MatView in, const float *mask, int num_seq, MatView out) {
  const int C = in.cols;
  const long long total = (long long)in.rows * C;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int r = (int)(e / C), c = (int)(e % C);
    out.data[(long long)r * out.stride + c] = in.data[(long long)r * in.stride + c] * mask[(long long)(r % num_seq) * C + c];
  }
}

__global__ __launch_bounds__(256) void dot_partial_kernel(const float *x, const float *y, size_t n, double *partial) {
  __shared__ double red[4];
  double s = 0;
  for (size_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (size_t)gridDim.x * 256ull) s += (double)x[i] * (double)y[i];
  s = block_sum256(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
__global__ void axpy_kernel(const float *x, float a, float *y, size_t n) {
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) y[i] += a * x[i];
}

}  // namespace
}  // namespace tdnnf

using namespace tdnnf;

extern "C" {

int tdnnf_relu_propagate(const tdnnf_mat *in, tdnnf_mat *out, tdnnf_stream stream) {
  TDNNF_REQUIRE(mat_ok(in) && mat_ok(out) && same_dim(in, out), "relu_propagate: bad matrices");
  TDNNF_HIP(launch_ew<0>(view(in), view(in), 0, 0, view(out), (hipStream_t)stream));
  return TDNNF_OK;
}
int tdnnf_relu_backprop(const tdnnf_mat *out_value, const tdnnf_mat *out_deriv, tdnnf_mat *in_deriv, tdnnf_stream stream) {
  TDNNF_REQUIRE(mat_ok(out_value) && mat_ok(out_deriv) && mat_ok(in_deriv) && same_dim(out_value, out_deriv) && same_dim(out_value, in_deriv),
                "relu_backprop: bad matrices");
  TDNNF_HIP(launch_ew<1>(view(out_value), view(out_deriv), 0, 0, view(in_deriv), (hipStream_t)stream));
  return TDNNF_OK;
}
int tdnnf_relu_repair(const double *stats, int dim, float self_repair_scale, float lower, float upper, tdnnf_mat *in_deriv, tdnnf_stream stream) {
  TDNNF_REQUIRE(stats && mat_ok(in_deriv) && in_deriv->cols == dim, "relu_repair: bad arguments");
  TDNNF_REQUIRE(self_repair_scale >= 0.0f && self_repair_scale < 0.1f, "relu_repair: self-repair-scale out of range");
  if (in_deriv->rows == 0) return TDNNF_OK;
  hipLaunchKernelGGL(relu_repair_kernel, dim3(grid_for((long long)in_deriv->rows * dim, 256)), dim3(256), 0, (hipStream_t)stream, stats, dim, self_repair_scale, lower, upper, view(in_deriv));
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}
int tdnnf_relu_store_stats(const tdnnf_mat *out_value, double *stats, void *ws, size_t ws_bytes, tdnnf_stream stream) {
  TDNNF_REQUIRE(mat_ok(out_value) && stats, "relu_store_stats: bad arguments");
  if (out_value->rows == 0) return TDNNF_OK;
  TDNNF_REQUIRE(ws && ws_bytes >= colreduce_bytes(out_value->rows, out_value->cols), "relu_store_stats: workspace too small");
  MatView a = view(out_value);
  ColReducePlan pl = colreduce_plan(a.rows, a.cols);
  TDNNF_HIP(colreduce_partial(3, a, a, (float *)ws, (hipStream_t)stream));
  hipLaunchKernelGGL(relu_stats_finalize_kernel, dim3((a.cols + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float *)ws, pl.chunks, a.cols, a.rows, stats);
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

int tdnnf_sum_scaled(const tdnnf_mat *a, float sa, const tdnnf_mat *b, float sb, tdnnf_mat *out, tdnnf_stream stream) {
  TDNNF_REQUIRE(mat_ok(a) && mat_ok(out) && same_dim(a, out) && (!b || (mat_ok(b) && same_dim(b, out))), "sum_scaled: bad matrices");
  if (b) TDNNF_HIP(launch_ew<2>(view(a), view(b), sa, sb, view(out), (hipStream_t)stream));
  else TDNNF_HIP(launch_ew<3>(view(a), view(a), sa, 0, view(out), (hipStream_t)stream));
  return TDNNF_OK;
}
int tdnnf_add_scaled(const tdnnf_mat *a, float sc, tdnnf_mat *out, tdnnf_stream stream) {
  TDNNF_REQUIRE(mat_ok(a) && mat_ok(out) && same_dim(a, out), "add_scaled: bad matrices");
  TDNNF_HIP(launch_ew<4>(view(a), view(a), sc, 0, view(out), (hipStream_t)stream));
  return TDNNF_OK;
}
int tdnnf_general_dropout(const tdnnf_mat *in, const float *mask, int num_seq, tdnnf_mat *out, tdnnf_stream stream) {
  TDNNF_REQUIRE(mat_ok(in) && mat_ok(out) && same_dim(in, out) && mask && num_seq > 0 && in->rows % num_seq == 0, "general_dropout: bad arguments");
  if (in->rows == 0) return TDNNF_OK;
  hipLaunchKernelGGL(dropout_kernel, dim3(grid_for((long long)in->rows * in->cols, 256)), dim3(256), 0, (hipStream_t)stream, view(in), mask, num_seq, view(out));
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

int tdnnf_general_dropout_mask(const float *uniform, long long n, float proportion, int continuous, float *mask, tdnnf_stream stream) {
  TDNNF_REQUIRE(n >= 0 && (n == 0 || (uniform && mask)) && proportion >= 0.f && proportion < 1.f, "general_dropout_mask: bad arguments (proportion in [0, 1))");
  if (n == 0) return TDNNF_OK;
  hipLaunchKernelGGL(general_dropout_mask_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, uniform, n, proportion, continuous, mask);
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

// UpdatableComponent::DotProduct (e.g. /root/reference/src/nnet3/nnet-tdnn-component.cc:949-958: TraceMatMat + VecVec): <x, y> in double
// over two device vectors; the result goes to the host, so the call synchronises the stream (model combination / diagnostics, not the
// training step).  Two stages, fixed order: 256 block partials, then the host adds them.
int tdnnf_dot(const float *x, const float *y, size_t n, double *result_host, tdnnf_stream stream) {
  TDNNF_REQUIRE(result_host && (n == 0 || (x && y)), "dot: null pointer");
  *result_host = 0.0;
  if (n == 0) return TDNNF_OK;
  constexpr int kBlocks = 256;
  double *partial = nullptr;
  TDNNF_HIP(hipMalloc((void **)&partial, sizeof(double) * kBlocks));
  hipLaunchKernelGGL(dot_partial_kernel, dim3(kBlocks), dim3(256), 0, (hipStream_t)stream, x, y, n, partial);
  double host[kBlocks];
  hipError_t e = hipMemcpyAsync(host, partial, sizeof(host), hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  (void)hipFree(partial);
  TDNNF_HIP(e);
  double acc = 0;
  for (int i = 0; i < kBlocks; i++) acc += host[i];
  *result_host = acc;
  return TDNNF_OK;
}

int tdnnf_axpy(const float *x, float a, float *y, size_t n, tdnnf_stream stream) {
  TDNNF_REQUIRE(x && y, "axpy: null pointer");
  if (n == 0 || a == 0.0f) return TDNNF_OK;
  hipLaunchKernelGGL(axpy_kernel, dim3(grid_for((long long)n, 256)), dim3(256), 0, (hipStream_t)stream, x, a, y, n);
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

}  // extern "C"
