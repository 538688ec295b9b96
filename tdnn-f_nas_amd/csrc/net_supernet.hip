// net_supernet.hip -- what a step (net_step.h) runs for the two supernets only: the bottleneck-dimension choice of a layer (forward: probabilities,
// column mask, masked linear output; backward: the C-vector's gradient and the masked derivative) and the tap coefficients of the offset
// (DARTS) supernet with the list of active taps.  Three host functions over five kernels, all on the stream they are given.
#include <math.h>
#include <string.h>

#include "net_step.h"

namespace tdnnf {
namespace {
// ---- bottleneck-dimension supernet (scripts/generate_bottleneckCB8share_onehottrain_config.py:10-85).
struct BnChoice {
  int C, mode;
  int cum[8];  // cumulative block widths: candidate bottleneck dims
  float flops_scale, temp;
};
// p (C): choice probabilities, identical for every row -- mode 0 OnehotFunctionComponent::Propagate
// (nnet-simple-component.cc:9504-9519), 1 SoftmaxFlops :9968-9981 on the ConstantFunction output, 2 GumbelSoftmaxFlops
// :10088-10113 (one noise vector shared by all rows).  mask[c] = sum_{j >= block(c)} p_j: CopyN of Sum(p_k..p_{C-1}).
__global__ void bn_choice_forward_kernel(BnChoice bc, const float *alpha, const float *u, float *p, float *mask) {
  __shared__ float sp[8];
  if (threadIdx.x == 0) {
    const int C = bc.C;
    if (bc.mode == 0) {
      for (int i = 0; i < C; i++) sp[i] = (u[0] >= (float)i / C && u[0] < (float)(i + 1) / C) ? 1.0f : 0.0f;
    } else {
      float v[8], mx = -INFINITY;
      for (int i = 0; i < C; i++) {
        v[i] = bc.mode == 2 ? (alpha[i] + -logf(-logf(u[i]))) * (1.0f / bc.temp) : alpha[i];
        mx = fmaxf(mx, v[i]);
      }
      double sum = 0;
      for (int i = 0; i < C; i++) sum += exp((double)v[i] - mx);
      for (int i = 0; i < C; i++) {
        const float q = (float)(exp((double)v[i] - mx) / sum);
        sp[i] = q < 1.0e-20f ? 1.0e-20f : q;  // ApplyFloor(1e-20)
      }
    }
    for (int i = 0; i < C; i++) p[i] = sp[i];
  }
  __syncthreads();
  const int bn = bc.cum[bc.C - 1];
  for (int c = threadIdx.x; c < bn; c += blockDim.x) {
    int k = 0;
    while (c >= bc.cum[k]) k++;
    float m = 0.f;
    for (int j = k; j < bc.C; j++) m += sp[j];  // Sum(softmax_k, ..., softmax_{C-1}) descriptor
    mask[c] = m;
  }
}
// out[r][c] = in[r][c] * mask[c]   (ElementwiseProductComponent :256-274 / :276-299 with a row-constant factor)
__global__ void col_scale_kernel(MatView in, const float *mask, MatView out) {
  const int C = in.cols;
  const long long total = (long long)in.rows * C;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int r = (int)(e / C), c = (int)(e % C);
    out.data[(size_t)r * out.stride + c] = in.data[(size_t)r * in.stride + c] * mask[c];
  }
}
// Gradient of the C-vector.  partial[chunk][c] = sum over the chunk's rows of lin[r][c] * d_masked[r][c]
// (ElementwiseProduct backprop w.r.t. the CopyN factor), E_j = sum_{c < cum[j]} (CopyN backprop + Sum descriptor).
//   mode 0: grad_j += E_j                                                    (OnehotFunction :9539-9548)
//   mode 1/2: e_j = E_j + flops_scale / C * (-cum[j]);  grad_j += 5 * p_j (e_j - <p, e>) / temp
//             ((Gumbel)SoftmaxFlops backprop summed over rows, then ConstantFunction :2636)
__global__ void bn_choice_backward_kernel(BnChoice bc, const float *partial, int chunks, const float *p, float *grad) {
  __shared__ double dm[512];
  const int bn = bc.cum[bc.C - 1];
  for (int c = threadIdx.x; c < bn; c += blockDim.x) {
    double sacc = 0;
    for (int k = 0; k < chunks; k++) sacc += partial[(size_t)k * bn + c];
    dm[c] = sacc;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double E[8], run = 0;
  int c = 0;
  for (int j = 0; j < bc.C; j++) {
    for (; c < bc.cum[j]; c++) run += dm[c];
    E[j] = run;
  }
  if (bc.mode == 0) {
    for (int j = 0; j < bc.C; j++) grad[j] += (float)E[j];
    return;
  }
  double pe = 0;
  for (int j = 0; j < bc.C; j++) {
    E[j] += (double)bc.flops_scale / bc.C * -(double)bc.cum[j];
    pe += (double)p[j] * E[j];
  }
  for (int j = 0; j < bc.C; j++) grad[j] += 5.0f * (float)(p[j] * (E[j] - pe)) * (1.0f / bc.temp);
}
// partial[chunk][c] = sum_{r in chunk} a[r][c] * b[r][c]
__global__ __launch_bounds__(256) void colsum_prod_partial_kernel(MatView a, MatView b, int rows_per_chunk, float *partial) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  const int r0 = blockIdx.y * rows_per_chunk, r1 = min(a.rows, r0 + rows_per_chunk);
  if (col >= a.cols) return;
  float sacc = 0.f;
  for (int r = r0; r < r1; r++) sacc += a.data[(size_t)r * a.stride + col] * b.data[(size_t)r * b.stride + col];
  partial[(size_t)blockIdx.y * a.cols + col] = sacc;
}
// active[0] = number of taps with a non-zero effective coefficient, active[1..] = their ids
__global__ void active_taps_kernel(const float *eff, int K, int *active) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int n = 0;
  for (int i = 0; i < K; i++)
    if (eff[i] != 0.f) active[1 + n++] = i;
  active[0] = n;
}

BnChoice bn_choice(const tdnnf_net_config &c) {
  BnChoice bc;
  memset(&bc, 0, sizeof(bc));
  bc.C = c.bn_num_choices;
  bc.mode = c.bn_mode;
  int run = 0;
  for (int k = 0; k < 8; k++) {
    if (k < bc.C) run += c.bn_choice_dims[k];
    bc.cum[k] = run;
  }
  bc.flops_scale = c.bn_flops_scale;
  bc.temp = c.bn_mode == 2 ? c.bn_temp_proportion : 1.0f;
  return bc;
}
}  // namespace

int darts_coef(tdnnf_net *n, TdnnfLayer &L, hipStream_t s) {
  const tdnnf_net_config &c = n->cfg;
  for (Tdnn *td : {&L.lin, &L.aff}) {
    const float *u = n->draws + td->draw0;
    CK(tdnnf_tdnn_darts_coef(net_alpha(n, td->comp), td->K, c.darts_flags, c.darts_temp_proportion, u, u + td->K, td->share, td->memo, darts_eff(*td), s));
    hipLaunchKernelGGL(active_taps_kernel, dim3(1), dim3(64), 0, s, darts_eff(*td), td->K, td->active);
  }
  return TDNNF_OK;
}
int bn_choice_forward(tdnnf_net *n, TdnnfLayer &L, hipStream_t s) {
  const tdnnf_net_config &c = n->cfg;
  TDNNF_REQUIRE(n->draws || c.bn_mode == 1, "net_forward_backward: the bottleneck supernet needs net_set_random_draws before every step");
  hipLaunchKernelGGL(bn_choice_forward_kernel, dim3(1), dim3(256), 0, s, bn_choice(c), net_W(n, L.c_arch),
                     n->draws ? n->draws + L.arch_draw0 : nullptr, L.arch_p, L.arch_mask);
  tdnnf_mat lin = M(L.lin_out, L.lin.rows_out, L.bn), masked = M(L.lin_masked, L.lin.rows_out, L.bn);
  hipLaunchKernelGGL(col_scale_kernel, dim3(grid_for((long long)lin.rows * L.bn, 256)), dim3(256), 0, s, view(&lin), L.arch_mask, view(&masked));
  return TDNNF_OK;
}
int bn_choice_backward(tdnnf_net *n, TdnnfLayer &L, tdnnf_mat &d_lin, hipStream_t s) {
  const int nl = L.lin.rows_out, chunks = (nl + 511) / 512;
  tdnnf_mat lin = M(L.lin_out, nl, L.bn);
  hipLaunchKernelGGL(colsum_prod_partial_kernel, dim3((L.bn + 255) / 256, chunks), dim3(256), 0, s, view(&lin), view(&d_lin), 512, (float *)n->ws);
  hipLaunchKernelGGL(bn_choice_backward_kernel, dim3(1), dim3(256), 0, s, bn_choice(n->cfg), (const float *)n->ws, chunks, L.arch_p, net_Wg(n, L.c_arch));
  hipLaunchKernelGGL(col_scale_kernel, dim3(grid_for((long long)nl * L.bn, 256)), dim3(256), 0, s, view(&d_lin), L.arch_mask, view(&d_lin));
  return TDNNF_OK;
}

}  // namespace tdnnf
