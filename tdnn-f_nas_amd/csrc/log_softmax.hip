// log_softmax.hip -- LogSoftmaxComponent, one 256-thread block per row (grid-stride over the rows, at most 8192 blocks): a one-pass form
// that holds the row in registers where the views allow 16-byte accesses and the row fits, a three-pass form for everything else, and the
// trainer's forward pass that also leaves a scaled softmax (log_softmax_propagate_with_aux, common.h).
//
// Reference: /root/reference/src/nnet3/nnet-simple-component.cc (exact line ranges are next to each C-ABI entry in include/tdnnf_hip.h).
#include <initializer_list>

#include "common.h"
#include "ew_dev.h"

namespace tdnnf {
namespace {

__global__ __launch_bounds__(256) void log_softmax_fwd_kernel(MatView in, MatView out) {
  __shared__ float red[4];
  for (int r = blockIdx.x; r < in.rows; r += gridDim.x) {
    const float *x = in.data + (long long)r * in.stride;
    float *o = out.data + (long long)r * out.stride;
    float mx = -INFINITY;
    for (int c = threadIdx.x; c < in.cols; c += 256) mx = fmaxf(mx, x[c]);
    mx = block_max256(mx, red);
    __syncthreads();
    float s = 0.f;
    for (int c = threadIdx.x; c < in.cols; c += 256) s += expf(x[c] - mx);
    const float lse = mx + logf(block_sum256(s, red));
    __syncthreads();
    for (int c = threadIdx.x; c < in.cols; c += 256) o[c] = x[c] - lse;
  }
}
// One pass per row with the row held in registers (up to 256 * 4 * NV columns, 16-byte aligned rows): the 6034-wide output
// rows are read once and written once instead of three reads through L2.
template <int NV>
__global__ __launch_bounds__(256) void log_softmax_fwd_regs_kernel(MatView in, MatView out, MatView aux, float aux_scale) {
  __shared__ float red[2][4];
  const int t = threadIdx.x, nc4 = (in.cols + 3) / 4;
  for (int r = blockIdx.x; r < in.rows; r += gridDim.x) {
    const float *x = in.data + (long long)r * in.stride;
    float *o = out.data + (long long)r * out.stride;
    float4 v[NV];
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < NV; k++) {
      const int c4 = t + 256 * k, c = c4 * 4;
      v[k] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
      if (c4 < nc4) ld4_ragged(x, c, in.cols, v[k]);
      mx = fmaxf(mx, fmaxf(fmaxf(v[k].x, v[k].y), fmaxf(v[k].z, v[k].w)));
    }
    mx = block_max256(mx, red[0]);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NV; k++) s += expf(v[k].x - mx) + expf(v[k].y - mx) + expf(v[k].z - mx) + expf(v[k].w - mx);  // exp(-inf) = 0 for the padding
    const float lse = mx + logf(block_sum256(s, red[1]));
#pragma unroll
    for (int k = 0; k < NV; k++) {
      const int c4 = t + 256 * k, c = c4 * 4;
      if (c4 >= nc4) continue;
      st4_ragged(o, c, in.cols, v[k], [&](float x) { return x - lse; });
      if (aux.data)  // aux = aux_scale * softmax(in): the dense part of the backward pass for a derivative with a known row sum
        st4_ragged(aux.data + (long long)r * aux.stride, c, in.cols, v[k], [&](float x) { return aux_scale * expf(x - lse); });
    }
    __syncthreads();  // red[] is reused by the next row
  }
}

template <int NV>
__global__ __launch_bounds__(256) void log_softmax_bwd_regs_kernel(MatView y, MatView dy, MatView dx) {
  __shared__ float red[4];
  const int t = threadIdx.x, nc4 = (y.cols + 3) / 4;
  for (int r = blockIdx.x; r < y.rows; r += gridDim.x) {
    const float *yv = y.data + (long long)r * y.stride, *e = dy.data + (long long)r * dy.stride;
    float *d = dx.data + (long long)r * dx.stride;
    float4 ev[NV], pv[NV];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NV; k++) {
      const int c4 = t + 256 * k, c = c4 * 4;
      ev[k] = pv[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c4 < nc4) {
        float4 q = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);  // exp(-inf) = 0 for the padding
        ld4_ragged(e, c, y.cols, ev[k]);
        ld4_ragged(yv, c, y.cols, q);
        pv[k] = make_float4(expf(q.x), expf(q.y), expf(q.z), expf(q.w));
      }
      s += (ev[k].x + ev[k].y) + (ev[k].z + ev[k].w);
    }
    s = block_sum256(s, red);
#pragma unroll
    for (int k = 0; k < NV; k++) {
      const int c4 = t + 256 * k, c = c4 * 4;
      if (c4 >= nc4) continue;
      st4_ragged(d, c, y.cols, make_float4(ev[k].x - pv[k].x * s, ev[k].y - pv[k].y * s, ev[k].z - pv[k].z * s, ev[k].w - pv[k].w * s));
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void log_softmax_bwd_kernel(MatView y, MatView dy, MatView dx) {
  __shared__ float red[4];
  for (int r = blockIdx.x; r < y.rows; r += gridDim.x) {
    const float *yv = y.data + (long long)r * y.stride, *e = dy.data + (long long)r * dy.stride;
    float *d = dx.data + (long long)r * dx.stride;
    float s = 0.f;
    for (int c = threadIdx.x; c < y.cols; c += 256) s += e[c];
    s = block_sum256(s, red);
    __syncthreads();
    for (int c = threadIdx.x; c < y.cols; c += 256) d[c] = e[c] - expf(yv[c]) * s;
  }
}

// float4s per thread of the one-pass kernels for rows of `cols` floats in these views: 2 or 8, or 0 where the three-pass kernel has to
// run (a view whose rows are not 16-byte aligned, or more than 256 * 4 * 8 columns)
int regs_nv(std::initializer_list<const tdnnf_mat *> views, int cols) {
  for (const tdnnf_mat *m : views)
    if (m->stride % 4 != 0 || ((uintptr_t)m->data & 15) != 0) return 0;
  return cols <= 256 * 4 * 2 ? 2 : cols <= 256 * 4 * 8 ? 8 : 0;
}
dim3 row_grid(int rows) { return dim3(rows < 8192 ? rows : 8192); }

void launch_fwd_regs(int nv, const tdnnf_mat *in, const tdnnf_mat *out, MatView aux, float aux_scale, hipStream_t s) {
  if (nv == 2) hipLaunchKernelGGL((log_softmax_fwd_regs_kernel<2>), row_grid(in->rows), dim3(256), 0, s, view(in), view(out), aux, aux_scale);
  else hipLaunchKernelGGL((log_softmax_fwd_regs_kernel<8>), row_grid(in->rows), dim3(256), 0, s, view(in), view(out), aux, aux_scale);
}

}  // namespace

// For an output derivative dy whose rows all sum to the same known c (xent_regularize * weight * numerator posteriors), the backward
// pass dy - softmax * rowsum(dy) is aux (aux_scale = -c) plus dy's few non-zeros added on top: no zero fill, no second dense pass.
bool log_softmax_propagate_with_aux(const tdnnf_mat *in, tdnnf_mat *out, tdnnf_mat *aux, float aux_scale, hipStream_t s) {
  const int nv = regs_nv({in, out, aux}, in->cols);
  if (nv == 0 || in->rows == 0) return false;
  launch_fwd_regs(nv, in, out, view(aux), aux_scale, s);
  return true;
}

}  // namespace tdnnf

using namespace tdnnf;

extern "C" {

int tdnnf_log_softmax_propagate(const tdnnf_mat *in, tdnnf_mat *out, tdnnf_stream stream) {
  TDNNF_REQUIRE(mat_ok(in) && mat_ok(out) && same_dim(in, out) && in->cols > 0, "log_softmax_propagate: bad matrices");
  if (in->rows == 0) return TDNNF_OK;
  if (const int nv = regs_nv({in, out}, in->cols)) launch_fwd_regs(nv, in, out, MatView{nullptr, 0, 0, 0}, 0.f, (hipStream_t)stream);
  else hipLaunchKernelGGL(log_softmax_fwd_kernel, row_grid(in->rows), dim3(256), 0, (hipStream_t)stream, view(in), view(out));
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

int tdnnf_log_softmax_backprop(const tdnnf_mat *out_value, const tdnnf_mat *out_deriv, tdnnf_mat *in_deriv, tdnnf_stream stream) {
  TDNNF_REQUIRE(mat_ok(out_value) && mat_ok(out_deriv) && mat_ok(in_deriv) && same_dim(out_value, out_deriv) && same_dim(out_value, in_deriv),
                "log_softmax_backprop: bad matrices");
  if (out_value->rows == 0) return TDNNF_OK;
  const dim3 grid = row_grid(out_value->rows);
  const int nv = regs_nv({out_value, out_deriv, in_deriv}, out_value->cols);
  if (nv == 2) hipLaunchKernelGGL((log_softmax_bwd_regs_kernel<2>), grid, dim3(256), 0, (hipStream_t)stream, view(out_value), view(out_deriv), view(in_deriv));
  else if (nv == 8) hipLaunchKernelGGL((log_softmax_bwd_regs_kernel<8>), grid, dim3(256), 0, (hipStream_t)stream, view(out_value), view(out_deriv), view(in_deriv));
  else hipLaunchKernelGGL(log_softmax_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, view(out_value), view(out_deriv), view(in_deriv));
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

}  // extern "C"
