// ng_group_kernels.h -- kernels and device-side descriptors of the grouped natural-gradient side chain and of the grouped finalize
// (ng_group.hip has the stages and the host code; the grouped GEMM stages are ggemm.h's).  Every launch runs over a descriptor table
// in device memory: one PairDesc per (component, side), one CompDesc per component, one FinDesc per refreshed object.
// Included into ng_group.hip's anonymous namespace, behind ggemm.h (f32x16).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "ggemm.h"

namespace tdnnf {
namespace {

// ------------------------------------------------------------------------------------------------ L = H^T H, traces, scale
struct PairDesc {  // one (component, side)
  const float *H;
  const double *part;  // ||X||^2 partials of the pass that formed H
  float *Ld;
  const float *WWT;
  double *scal;
  float *scale_f;
  // refresh
  const float *Kd;
  float *hK, *hL;  // pinned host memory (device-visible)
  double *h_tr0;
  double ones_term;
  int N, Rp, nt, npart;
  int slab0, nslab, rows_per_slab;
};
__device__ __forceinline__ int ntile_pairs(int nt) { return nt * (nt + 1) / 2; }
// floats of one slab's partial: the raw accumulator images (16 registers x 64 lanes) of up to six tile pairs (nt <= 3)
constexpr int kLSlabFloats = 6 * 1024;

// block -> descriptor, for launches whose descriptors own consecutive block ranges: the last i in [0, n) with d[i].*Start <= blk
template <auto Start, class Desc>
__device__ __forceinline__ int last_start_le(const Desc *d, int n, int blk) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (d[mid].*Start <= blk) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// block (pair, slab): the slab's contribution to the upper-triangular 32 x 32 tiles of H^T H, as raw accumulator images
// [tile pair][register][lane].  A wave takes every fourth pair of rows; lane (li, lh) holds H[row + lh][32 c + li] for the
// column tiles c, which is both the A fragment (A[i = li][k = lh]) and the B fragment (B[k = lh][j = li]) of the MFMA.
template <int NT>
__device__ __forceinline__ void l_partial_body(const PairDesc &p, int slab, float *partial, float *lds) {
  constexpr int NP = NT * (NT + 1) / 2;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 31, lh = lane >> 5;
  const int Rp = p.Rp, r0 = slab * p.rows_per_slab, r1 = min(p.N, r0 + p.rows_per_slab);
  f32x16 acc[NP];
#pragma unroll
  for (int q = 0; q < NP; q++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[q][r] = 0.f;
  bool cv[NT];
#pragma unroll
  for (int c = 0; c < NT; c++) cv[c] = c * 32 + li < Rp;
  constexpr int U = 4;  // pairs of rows requested together
  for (int base = r0 + 2 * wave; base < r1; base += 8 * U) {
    float a[U][NT];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int row = base + 8 * u + lh;
      const float *h = p.H + (size_t)row * Rp + li;
#pragma unroll
      for (int c = 0; c < NT; c++) a[u][c] = (row < r1 && cv[c]) ? h[c * 32] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      int q = 0;
#pragma unroll
      for (int i = 0; i < NT; i++)
#pragma unroll
        for (int j = i; j < NT; j++, q++) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][i], a[u][j], acc[q], 0, 0, 0);
    }
  }
  // waves 2, 3 -> LDS, waves 0, 1 add; wave 1 -> LDS, wave 0 adds and stores (fixed order)
  float *mine = lds + (size_t)(wave & 1) * NP * 1024;
  if (wave >= 2) {
#pragma unroll
    for (int q = 0; q < NP; q++)
#pragma unroll
      for (int r = 0; r < 16; r++) mine[(q * 16 + r) * 64 + lane] = acc[q][r];
  }
  __syncthreads();
  if (wave < 2) {
#pragma unroll
    for (int q = 0; q < NP; q++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[q][r] += mine[(q * 16 + r) * 64 + lane];
  }
  __syncthreads();
  if (wave == 1) {
#pragma unroll
    for (int q = 0; q < NP; q++)
#pragma unroll
      for (int r = 0; r < 16; r++) lds[(q * 16 + r) * 64 + lane] = acc[q][r];
  }
  __syncthreads();
  if (wave == 0) {
    float *out = partial + (size_t)(p.slab0 + slab) * kLSlabFloats;
#pragma unroll
    for (int q = 0; q < NP; q++)
#pragma unroll
      for (int r = 0; r < 16; r++) out[(q * 16 + r) * 64 + lane] = acc[q][r] + lds[(q * 16 + r) * 64 + lane];
  }
}

__global__ __launch_bounds__(256) void ng_l_partial_kernel(const PairDesc *pairs, int npairs, float *partial) {
  extern __shared__ float lds[];
  const PairDesc &p = pairs[last_start_le<&PairDesc::slab0>(pairs, npairs, (int)blockIdx.x)];  // block -> (pair, slab)
  const int slab = blockIdx.x - p.slab0;
  if (p.nt == 1) l_partial_body<1>(p, slab, partial, lds);
  else if (p.nt == 2) l_partial_body<2>(p, slab, partial, lds);
  else l_partial_body<3>(p, slab, partial, lds);
}

// one block (1024 threads: an accumulator image per pass) per (component, side): L from the slab partials (slabs added in order), then
//   tr0 = sum ||X||^2 partials + ones_term,  tr1 = tr0 - 2 tr(L) + <L, W W^T>,  scale = sqrt(tr0 / tr1)
__global__ __launch_bounds__(1024) void ng_l_finish_kernel(const PairDesc *pairs, const float *partial) {
  __shared__ double red[3][16];
  const PairDesc &p = pairs[blockIdx.x];
  const int t = threadIdx.x, Rp = p.Rp, nt = p.nt;
  double a = 0, b = 0, c = 0;
  for (int i = t; i < p.npart; i += 1024) a += p.part[i];
  int q = 0;
  for (int ti = 0; ti < nt; ti++)
    for (int tj = ti; tj < nt; tj++, q++) {
      const int e = t, r = e >> 6, lane = e & 63;
      const int m = ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), n = tj * 32 + (lane & 31);
      if (m >= Rp || n >= Rp) continue;
      const float *src = partial + (size_t)p.slab0 * kLSlabFloats + (size_t)q * 1024 + e;
      float v = 0.f;
      int s = 0;
      for (; s + 7 < p.nslab; s += 8) {
        float w[8];
#pragma unroll
        for (int u = 0; u < 8; u++) w[u] = src[(size_t)(s + u) * kLSlabFloats];
#pragma unroll
        for (int u = 0; u < 8; u++) v += w[u];
      }
      for (; s < p.nslab; s++) v += src[(size_t)s * kLSlabFloats];
      p.Ld[m * Rp + n] = v;
      const double w = (double)v * (double)p.WWT[m * Rp + n];
      if (ti != tj) {
        p.Ld[n * Rp + m] = v;
        c += 2.0 * w;
      } else {
        c += w;
        if (m == n) b += v;
      }
    }
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
    c += __shfl_xor(c, o, 64);
  }
  if ((t & 63) == 0) {
    red[0][t >> 6] = a;
    red[1][t >> 6] = b;
    red[2][t >> 6] = c;
  }
  __syncthreads();
  if (t == 0) {
    double tr0 = p.ones_term, trL = 0, trLW = 0;
    for (int w = 0; w < 16; w++) {
      tr0 += red[0][w];
      trL += red[1][w];
      trLW += red[2][w];
    }
    const double tr1 = tr0 - 2.0 * trL + trLW;
    p.scal[0] = tr0;
    p.scal[1] = tr1;
    *p.scale_f = (tr0 <= 0.0 || !(tr1 > 0.0)) ? 1.0f : (float)sqrt(tr0 / tr1);
  }
}

// refresh: K, L and tr(XX^T) of every pair to the pinned buffers the pool threads read
__global__ __launch_bounds__(256) void ng_stage_kernel(const PairDesc *pairs) {
  const PairDesc &p = pairs[blockIdx.x];
  const int n = p.Rp * p.Rp;
  for (int i = threadIdx.x; i < n; i += 256) {
    p.hK[i] = p.Kd[i];
    p.hL[i] = p.Ld[i];
  }
  if (threadIdx.x == 0) *p.h_tr0 = p.scal[0];
}

// ------------------------------------------------------------------------------------------------ per-component stages
struct CompDesc {
  float *T;
  const float *bsum, *sa, *sb;
  float *W_acc, *bias_acc;
  int Do, ldT, ldw, Dx;
  int blk0;  // first block of this component in the commit launch
};
// T[o][ldw] = bsum[o], zeros in the row padding (one block per component)
__global__ __launch_bounds__(256) void ng_set_columns_kernel(const CompDesc *comps) {
  const CompDesc &c = comps[blockIdx.x];
  if (!c.bsum && c.ldT == c.ldw) return;
  for (int o = threadIdx.x; o < c.Do; o += 256) {
    float *row = c.T + (size_t)o * c.ldT;
    int col = c.ldw;
    if (c.bsum) row[col++] = c.bsum[o];
    for (; col < c.ldT; col++) row[col] = 0.f;
  }
}
// W_acc[o][c] += a b T[o][c] (c < ldw), bias_acc[o] += a b T[o][ldw]: "local_lrate = scale * learning_rate_"
// (nnet-tdnn-component.cc:604-624); a, b: the two preconditioners' scales, on the device.  1024 elements per block.
__global__ __launch_bounds__(256) void ng_commit_group_kernel(const CompDesc *comps, int ncomps) {
  const int ci = last_start_le<&CompDesc::blk0>(comps, ncomps, blockIdx.x);
  const CompDesc &c = comps[ci];
  const float sc = c.sa[0] * c.sb[0];
  const int C = c.Dx;
  const long long total = (long long)c.Do * C, e0 = (long long)(blockIdx.x - c.blk0) * 1024;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const long long e = e0 + j * 256 + threadIdx.x;
    if (e >= total) break;
    const int o = (int)(e / C), col = (int)(e % C);
    const float v = sc * c.T[(size_t)o * c.ldT + col];
    if (col < c.ldw) c.W_acc[(size_t)o * c.ldw + col] += v;
    else c.bias_acc[o] += v;
  }
}

// ------------------------------------------------------------------------------------------------ grouped finalize
struct FinDesc {  // one refreshed object
  float *J, *W, *W1, *WT, *wlast;
  const float *h_coeff;  // pinned
  int Rp, D, Dp;
  int blk0;
};
// J[r][d] += coeff[r] W[r][d]   (B_t = J_t + (1 - eta) / (eta / N) (D_t + rho_t I) W_t)
__global__ __launch_bounds__(256) void ng_fin_adddiag_kernel(const FinDesc *f, int nf) {
  const FinDesc &p = f[last_start_le<&FinDesc::blk0>(f, nf, blockIdx.x)];
  const long long total = (long long)p.Rp * p.Dp, e0 = (long long)(blockIdx.x - p.blk0) * 1024;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const long long e = e0 + j * 256 + threadIdx.x;
    if (e >= total) break;
    p.J[e] += p.h_coeff[e / p.Dp] * p.W[e];
  }
}
// W = W1, W^T, last column
__global__ __launch_bounds__(256) void ng_fin_derive_kernel(const FinDesc *f, int nf) {
  const FinDesc &p = f[last_start_le<&FinDesc::blk0>(f, nf, blockIdx.x)];
  const long long total = (long long)p.Rp * p.Dp, e0 = (long long)(blockIdx.x - p.blk0) * 1024;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const long long e = e0 + j * 256 + threadIdx.x;
    if (e >= total) break;
    const int r = (int)(e / p.Dp), d = (int)(e % p.Dp);
    const float v = p.W1[e];
    p.W[e] = v;
    if (d < p.D) {
      p.WT[(size_t)d * p.Rp + r] = v;
      if (d == p.D - 1) p.wlast[r] = v;
    }
  }
}

}  // namespace
}  // namespace tdnnf
