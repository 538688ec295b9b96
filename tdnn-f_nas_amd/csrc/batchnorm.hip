// batchnorm.hip -- BatchNormComponent and BatchNormTestComponent as stand-alone passes (batchnorm.h): column statistics by the two-stage
// reduction (colreduce.h), a finalize launch for the memo rows, one apply pass; the thread-local scopes of synchronised BatchNorm and of
// the norm bound.  The trainer's fused forms are in fused.hip.
//
// Reference: /root/reference/src/nnet3/nnet-normalize-component.cc (exact line ranges are next to each C-ABI entry in
// include/tdnnf_hip.h).
#include "batchnorm.h"
#include "ew_dev.h"

namespace tdnnf {
namespace {

// BatchNormComponent::StoreStats (nnet-normalize-component.cc:551-589) for column d: count += I, sum += I mean, sumsq += I uvar
__device__ __forceinline__ void bn_store_stats(double *stats, int D, int d, int frames, float mean, float uvar) {
  if (d == 0) stats[0] += (double)frames;
  stats[1 + d] += (double)frames * mean;
  stats[1 + D + d] += (double)frames * uvar;
}

// finalize forward stats: memo rows 0 mean, 1 uvar, 2 scale  (nnet-normalize-component.cc:433-445)
// sums_out (synchronised BatchNorm, first half): only the column sums, as doubles [2][D].  sums_in (second half): the sums come
// from there (all-reduced over the ranks) instead of from the partial rows, and N is the global row count.
__global__ __launch_bounds__(kFinThreads) void bn_fwd_finalize_kernel(const float *partial, int chunks, int D, int N, float epsilon,
                                                                      float target_rms, float *memo, double *sums_out = nullptr,
                                                                      const double *sums_in = nullptr, double *store = nullptr, int store_frames = 0,
                                                                      double *fro2 = nullptr) {
  __shared__ double red[2 * kFinLanes * (kFinCols + 1)];
  const int d = blockIdx.x * kFinCols + (threadIdx.x & (kFinCols - 1));
  double q[2];
  if (!sums_in) finalize_sums<2, double>(partial, chunks, chunks, D, 2, q, red);
  const bool own = threadIdx.x < kFinCols && d < D;
  if (sums_out) {
    if (own) {
      sums_out[d] = q[0];
      sums_out[D + d] = q[1];
    }
    return;
  }
  double bound = 0;  // sum over rows of z^2 for this column: N scale^2 var (store_frames = this rank's rows)
  if (own) {
    if (sums_in) {
      q[0] = sums_in[d];
      q[1] = sums_in[D + d];
    }
    const float mean = (float)(q[0] / N), uvar = (float)(q[1] / N);
    const float var_scale = 1.0f / (target_rms * target_rms);
    float v = var_scale * uvar - var_scale * mean * mean;
    v = floor_keep_nan(v, 0.f) + var_scale * epsilon;
    memo[d] = mean;
    memo[D + d] = uvar;
    const float sc = 1.0f / sqrtf(v);
    memo[2 * D + d] = sc;
    const double var = (double)uvar - (double)mean * mean;
    bound = (double)N * sc * sc * (var > 0 ? var : 0.0);
    if (store) bn_store_stats(store, D, d, store_frames, mean, uvar);  // StoreStats in the same launch
  }
  if (fro2 && threadIdx.x < 64) {  // (the kFinCols <= 32 owning threads are the first lanes of the first wave; the other lanes carry zeros)
    for (int o = 16; o > 0; o >>= 1) bound += __shfl_xor(bound, o, 32);
    if (threadIdx.x == 0) fro2[blockIdx.x] = bound;
  }
}
// memo rows 3 var_deriv_mod, 4 temp (:520-526)
__global__ __launch_bounds__(kFinThreads) void bn_bwd_finalize_kernel(const float *partial, int chunks, int D, int N, float target_rms, float *memo,
                                                                      double *sums_out = nullptr, const double *sums_in = nullptr) {
  __shared__ double red[2 * kFinLanes * (kFinCols + 1)];
  const int d = blockIdx.x * kFinCols + (threadIdx.x & (kFinCols - 1));
  double q[2];
  if (!sums_in) finalize_sums<2, double>(partial, chunks, chunks, D, 2, q, red);
  if (threadIdx.x >= kFinCols || d >= D) return;
  if (sums_out) {
    sums_out[d] = q[0];
    sums_out[D + d] = q[1];
    return;
  }
  if (sums_in) {
    q[0] = sums_in[d];
    q[1] = sums_in[D + d];
  }
  const float coeff = -1.0f / (target_rms * target_rms * N);
  memo[3 * D + d] = (float)(coeff * q[0]) * memo[2 * D + d];
  memo[4 * D + d] = (float)(-q[1] / N);
}

// per-column affine maps.  MODE 1: out = in * mul[c] + add[c]                    (bn test fwd)
//                          MODE 2: out = in * mul[c]                             (bn test bwd; add unused)
//                          MODE 3: out = (in + add[c]) * mul[c] + z * vdm[c]     (bn train bwd)
// z and vdm are read by MODE 3 only.
template <int MODE, int VEC>
__global__ __launch_bounds__(256) void colmap_kernel(MatView in, MatView z, const float *mul, const float *add,
                                                     const float *vdm, MatView out) {
  static_assert(MODE >= 1 && MODE <= 3, "colmap_kernel: no such map");
  const int cv = in.cols / VEC;
  const long long total = (long long)in.rows * cv;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int r = (int)(e / cv), c = (int)(e % cv) * VEC;
    float x[4], zz[4], o[4];
    ld(in.data + (long long)r * in.stride + c, x, VEC == 4);
    if (MODE == 3) ld(z.data + (long long)r * z.stride + c, zz, VEC == 4);
#pragma unroll
    for (int j = 0; j < VEC; j++) {
      if (MODE == 1) o[j] = x[j] * mul[c + j] + add[c + j];
      if (MODE == 2) o[j] = x[j] * mul[c + j];
      if (MODE == 3) o[j] = fmaf(x[j] + add[c + j], mul[c + j], zz[j] * vdm[c + j]);  // (spelled out: the same roundings whatever VEC is)
    }
    st(out.data + (long long)r * out.stride + c, o, VEC == 4);
  }
}
// bn train fwd: out = (in - mean[c]) * scale[c]
template <int VEC>
__global__ __launch_bounds__(256) void bn_apply_kernel(MatView in, const float *mean, const float *scale, MatView out) {
  const int cv = in.cols / VEC;
  const long long total = (long long)in.rows * cv;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int r = (int)(e / cv), c = (int)(e % cv) * VEC;
    float v[4], m[4], sc[4];
    ld(in.data + (long long)r * in.stride + c, v, VEC == 4);
    ld(mean + c, m, VEC == 4);
    ld(scale + c, sc, VEC == 4);
#pragma unroll
    for (int j = 0; j < VEC; j++) v[j] = (v[j] - m[j]) * sc[j];
    st(out.data + (long long)r * out.stride + c, v, VEC == 4);
  }
}

__global__ void bn_store_stats_kernel(const float *memo, int D, int num_frames, double *stats) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d < D) bn_store_stats(stats, D, d, num_frames, memo[d], memo[D + d]);
}
__global__ void bn_derived_kernel(const double *stats, int D, float epsilon, float target_rms, float *scale,
                                  float *offset) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= D) return;
  const double count = stats[0];
  float off = (float)(stats[1 + d] * (-1.0 / count));
  float sc = (float)(stats[1 + D + d] * (1.0 / count));
  sc += -1.0f * off * off;
  sc = floor_keep_nan(sc, 0.f) + epsilon;
  sc = 1.0f / sqrtf(sc);
  sc *= target_rms;
  scale[d] = sc;
  offset[d] = off * sc;
}

thread_local double *g_fro_buf = nullptr;
thread_local int *g_fro_blocks = nullptr;
thread_local BnSync *g_bn_sync = nullptr;

// memo rows 0-2 from partial column sums; with a BnSync installed the sums are all-reduced over the ranks first
hipError_t bn_fwd_finalize(const float *partial, int chunks, int rows, int cols, float epsilon, float target_rms, float *memo, hipStream_t s,
                           double *store = nullptr) {
  double *fro2 = fro_bound_buf();
  if (fro2 && fro_bound_blocks()) *fro_bound_blocks() = (int)finalize_grid(cols);
  // (store and fro2 are read by the launch that forms the memo; with a BnSync its bound covers all ranks' rows: still an upper bound of this rank's)
  return bn_finalize_synced(bn_sync_current(), 2, cols, rows, s, [&](double *sums_out, const double *sums_in, int N) {
    hipLaunchKernelGGL(bn_fwd_finalize_kernel, dim3(finalize_grid(cols)), dim3(kFinThreads), 0, s, partial, chunks, cols, N, epsilon, target_rms, memo, sums_out,
                       sums_in, store, rows, fro2);
  });
}
hipError_t bn_bwd_finalize(const float *partial, int chunks, int rows, int D, float target_rms, float *memo, hipStream_t s) {
  return bn_finalize_synced(bn_sync_current(), 2, D, rows, s, [&](double *sums_out, const double *sums_in, int N) {
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(finalize_grid(D)), dim3(kFinThreads), 0, s, partial, chunks, D, N, target_rms, memo, sums_out, sums_in);
  });
}

}  // namespace

FroBoundScope::FroBoundScope(double *buf, int *blocks) : prev_buf(g_fro_buf), prev_blocks(g_fro_blocks) {
  g_fro_buf = buf;
  g_fro_blocks = blocks;
  if (blocks) *blocks = 0;
}
FroBoundScope::~FroBoundScope() {
  g_fro_buf = prev_buf;
  g_fro_blocks = prev_blocks;
}
double *fro_bound_buf() { return g_fro_buf; }
int *fro_bound_blocks() { return g_fro_blocks; }
BnSync *bn_sync_current() { return g_bn_sync; }
BnSyncScope::BnSyncScope(BnSync *b) : prev(g_bn_sync) { g_bn_sync = b; }
BnSyncScope::~BnSyncScope() { g_bn_sync = prev; }

hipError_t batchnorm_stats(MatView a, float epsilon, float target_rms, float *memo, void *ws, hipStream_t s, double *store_stats) {
  hipError_t e = colreduce_partial(1, a, a, (float *)ws, s);
  if (e != hipSuccess) return e;
  return bn_fwd_finalize((const float *)ws, colreduce_plan(a.rows, a.cols).chunks, a.rows, a.cols, epsilon, target_rms, memo, s, store_stats);
}
hipError_t batchnorm_stats_from_partials(const float *partial, int chunks, int rows, int cols, float epsilon, float target_rms, float *memo, hipStream_t s,
                                         double *store_stats) {
  return bn_fwd_finalize(partial, chunks, rows, cols, epsilon, target_rms, memo, s, store_stats);
}

}  // namespace tdnnf

using namespace tdnnf;

extern "C" {

int tdnnf_batchnorm_propagate(const tdnnf_mat *in, float epsilon, float target_rms, tdnnf_mat *out, float *memo,
                              void *ws, size_t ws_bytes, tdnnf_stream stream) {
  TDNNF_REQUIRE(mat_ok(in) && mat_ok(out) && same_dim(in, out) && memo, "batchnorm_propagate: bad matrices");
  TDNNF_REQUIRE(in->rows > 0 && epsilon > 0 && target_rms > 0, "batchnorm_propagate: empty input or bad epsilon/target-rms");
  TDNNF_REQUIRE(ws && ws_bytes >= colreduce_bytes(in->rows, in->cols), "batchnorm_propagate: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  MatView a = view(in), o = view(out);
  TDNNF_HIP(batchnorm_stats(a, epsilon, target_rms, memo, ws, s));
  const bool vec = vec4_ok(a) && vec4_ok(o) && (reinterpret_cast<uintptr_t>(memo) & 15) == 0;  // (memo rows as float4s)
  TDNNF_HIP(launch_vec_or_scalar(vec, a.rows, a.cols, bn_apply_kernel<4>, bn_apply_kernel<1>, s, a, memo, memo + 2 * a.cols, o));
  return TDNNF_OK;
}

int tdnnf_batchnorm_backprop(const tdnnf_mat *out_value, const tdnnf_mat *out_deriv, float target_rms, float *memo,
                             tdnnf_mat *in_deriv, void *ws, size_t ws_bytes, tdnnf_stream stream) {
  TDNNF_REQUIRE(mat_ok(out_value) && mat_ok(out_deriv) && mat_ok(in_deriv) && same_dim(out_value, out_deriv) &&
                    same_dim(out_value, in_deriv) && memo,
                "batchnorm_backprop: bad matrices");
  TDNNF_REQUIRE(out_value->rows > 0, "batchnorm_backprop: empty input");
  TDNNF_REQUIRE(ws && ws_bytes >= colreduce_bytes(out_value->rows, out_value->cols), "batchnorm_backprop: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  MatView z = view(out_value), dz = view(out_deriv), dx = view(in_deriv);
  const int D = z.cols;
  TDNNF_HIP(colreduce_partial(2, z, dz, (float *)ws, s));
  TDNNF_HIP(bn_bwd_finalize((const float *)ws, colreduce_plan(z.rows, D).chunks, z.rows, D, target_rms, memo, s));
  // dx = (dz + temp) * scale + z * vdm
  TDNNF_HIP(launch_vec_or_scalar(vec4_ok(z) && vec4_ok(dz) && vec4_ok(dx), z.rows, D, colmap_kernel<3, 4>, colmap_kernel<3, 1>, s, dz, z, memo + 2 * D, memo + 4 * D,
                                 memo + 3 * D, dx));
  return TDNNF_OK;
}

int tdnnf_batchnorm_store_stats(const float *memo, int D, int num_frames, double *stats, tdnnf_stream stream) {
  TDNNF_REQUIRE(memo && stats && D > 0 && num_frames > 0, "batchnorm_store_stats: bad arguments");
  hipLaunchKernelGGL(bn_store_stats_kernel, dim3((D + 255) / 256), dim3(256), 0, (hipStream_t)stream, memo, D, num_frames, stats);
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

int tdnnf_batchnorm_compute_derived(const double *stats, int D, float epsilon, float target_rms, float *scale,
                                    float *offset, tdnnf_stream stream) {
  TDNNF_REQUIRE(stats && scale && offset && D > 0, "batchnorm_compute_derived: bad arguments");
  hipLaunchKernelGGL(bn_derived_kernel, dim3((D + 255) / 256), dim3(256), 0, (hipStream_t)stream, stats, D, epsilon, target_rms, scale, offset);
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

int tdnnf_batchnorm_test_propagate(const tdnnf_mat *in, const float *scale, const float *offset, tdnnf_mat *out,
                                   tdnnf_stream stream) {
  TDNNF_REQUIRE(mat_ok(in) && mat_ok(out) && same_dim(in, out) && scale && offset, "batchnorm_test_propagate: bad arguments");
  MatView a = view(in), o = view(out);
  if (a.rows == 0) return TDNNF_OK;
  const MatView no_z{nullptr, 0, 0, 0};
  TDNNF_HIP(launch_vec_or_scalar(vec4_ok(a) && vec4_ok(o), a.rows, a.cols, colmap_kernel<1, 4>, colmap_kernel<1, 1>, (hipStream_t)stream, a, no_z, scale, offset,
                                 (const float *)nullptr, o));
  return TDNNF_OK;
}

int tdnnf_batchnorm_test_backprop(const tdnnf_mat *out_deriv, const float *scale, tdnnf_mat *in_deriv, tdnnf_stream stream) {
  TDNNF_REQUIRE(mat_ok(out_deriv) && mat_ok(in_deriv) && same_dim(out_deriv, in_deriv) && scale, "batchnorm_test_backprop: bad arguments");
  MatView a = view(out_deriv), o = view(in_deriv);
  if (a.rows == 0) return TDNNF_OK;
  const MatView no_z{nullptr, 0, 0, 0};
  TDNNF_HIP(launch_vec_or_scalar(vec4_ok(a) && vec4_ok(o), a.rows, a.cols, colmap_kernel<2, 4>, colmap_kernel<2, 1>, (hipStream_t)stream, a, no_z, scale,
                                 (const float *)nullptr, (const float *)nullptr, o));
  return TDNNF_OK;
}

}  // extern "C"
