// den_persistent_kernels.h -- the denominator with ONE persistent workgroup per sequence (chain_types.h): forward and backward
// recursion, the self-normalised backward recursion that runs beside the forward one, and the occupancy pass over all frames
// (one or two frames per workgroup).  Launched by chain_den.hip only.
#pragma once
#include "den_dev.h"

namespace tdnnf {
namespace {

// Forward: alpha_dash(t, .) for t = 0..T stored to `alpha` [(T+1) x Hs] per sequence, alpha sums to
// `asum` [T+1], per-sequence log-prob to logprob[s].
// FAST (the host checks: state vectors in LDS, at most kDenFastSlots rows and kDenFastStates states per thread): everything that does not change from
// frame to frame -- a thread's slices, rows and initial probabilities -- stays in registers, and a frame's new vector is formed in a second LDS
// buffer: no load inside a frame depends on another load or store of the same frame except the arcs themselves (the plain loop re-reads the slice
// table, the row ids, init[] and -- after a global store -- its own alpha row, each a trip to L2 in front of the next barrier).
// res_cap > 0: the first res_cap arcs of the table (its widest slices) stay in LDS for all frames -- used when the launch holds every CU anyway.
constexpr int kDenFastSlots = 4, kDenFastStates = 4;  // (both tables of these kernels have one row per state)
template <bool LDS_STATE, bool FAST = false>
__global__ __launch_bounds__(kDenThreads) void den_forward_kernel(DenDev g, MatView y, int B, int T, float leaky,
                                                                  float *alpha_all, float *asum_all, int Hs,
                                                                  double *logprob, float *gstate, const unsigned *only_if, int res_cap) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float red[kDenThreads / 64];
  if (only_if && *only_if == 0) return;  // fallback launch behind the multi-workgroup recursion: runs only when that one gave up
  const int s = blockIdx.x, tid = threadIdx.x;
  const int H = g.H, P = g.P;
  float *x = smem;  // P
  float *prev = LDS_STATE ? smem + ((P + 3) & ~3) : gstate + (size_t)s * 2 * Hs;
  float *nxt = smem + ((P + 3) & ~3) + Hs;  // FAST: the frame's new vector
  uint2 *lres = reinterpret_cast<uint2 *>(smem + ((P + 3) & ~3) + (LDS_STATE ? Hs : 0) + (FAST ? Hs : 0));
  for (int i = tid; i < res_cap; i += kDenThreads) lres[i] = g.by_dst.arc[i];
  int sb0[kDenFastSlots], sw[kDenFastSlots];
  unsigned srow[kDenFastSlots];
  float hinit[kDenFastStates];
  if constexpr (FAST) {
#pragma unroll
    for (int k = 0; k < kDenFastSlots; k++) {
      const int slot = tid + k * kDenThreads;
      sb0[k] = 0;
      sw[k] = 0;
      srow[k] = 0xffffffffu;
      if (slot < g.by_dst.nslices * 64) {
        sb0[k] = g.by_dst.base[slot >> 6];
        sw[k] = (g.by_dst.base[(slot >> 6) + 1] - sb0[k]) >> 6;
        srow[k] = g.by_dst.row[slot];
      }
    }
#pragma unroll
    for (int i = 0; i < kDenFastStates; i++) hinit[i] = tid + i * kDenThreads < H ? g.init[tid + i * kDenThreads] : 0.f;
  }
  float *alpha = alpha_all + (size_t)s * (T + 1) * Hs;
  float *asum = asum_all + (size_t)s * (T + 1);

  // AlphaFirstFrame + AlphaDash(0)
  for (int h = tid; h < H; h += kDenThreads) {
    const float a = g.init[h] + leaky * g.init_sum * g.init[h];
    prev[h] = a;
    alpha[h] = a;
  }
  if (tid == 0) asum[0] = g.init_sum;
  float prev_sum = g.init_sum;
  double logcorr = 0.0;
  RowAhead ra;
  ra.load(y.data + (size_t)s * y.stride, P, tid);
  __syncthreads();
  for (int t = 1; t <= T; t++) {
#pragma unroll
    for (int i = 0; i < kDenRowRegs; i++)
      if (tid + i * kDenThreads < P) x[tid + i * kDenThreads] = exp_limited(ra.v[i]);
    for (int p = tid + kDenRowRegs * kDenThreads; p < P; p += kDenThreads) x[p] = exp_limited(y.data[(size_t)((t - 1) * B + s) * y.stride + p]);  // (more than 8 192 pdfs: the rest as before)
    if (t < T) ra.load(y.data + (size_t)(t * B + s) * y.stride, P, tid);  // the next frame's row: lands while this frame's arcs are walked
    __syncthreads();
    const float inv = 1.0f / prev_sum;
    logcorr += (double)logf(prev_sum);
    float *cur = alpha + (size_t)t * Hs;
    float local = 0.f;
    auto term = [&](const uint2 a) { return prev[a.x & 0xffffu] * __uint_as_float(a.y) * x[a.x >> 16]; };
    if constexpr (FAST) {
      const int ln = tid & 63;
#pragma unroll
      for (int k = 0; k < kDenFastSlots; k++) {
        if (srow[k] == 0xffffffffu && sw[k] == 0) continue;
        float acc = sb0[k] + sw[k] * 64 <= res_cap ? sell_row_sum(lres + sb0[k] + ln, sw[k], term) : sell_row_sum(g.by_dst.arc + sb0[k] + ln, sw[k], term);
        if (srow[k] != 0xffffffffu) {
          acc *= inv;
          nxt[srow[k]] = acc;  // alpha(t,h) before the leaky term
          local += acc;
        }
      }
      const float sum = block_sum(local, red, kDenThreads / 64);  // (its barriers: every row of nxt is written)
      if (tid == 0) asum[t] = sum;
#pragma unroll
      for (int i = 0; i < kDenFastStates; i++) {  // AlphaDash(t)
        const int h = tid + i * kDenThreads;
        if (h < H) {
          const float a = nxt[h] + leaky * sum * hinit[i];
          nxt[h] = a;
          cur[h] = a;
        }
      }
      float *other = prev;
      prev = nxt;
      nxt = other;
      prev_sum = sum;
      __syncthreads();
      continue;
    }
    for (int slot = tid; slot < g.by_dst.nslices * 64; slot += kDenThreads) {
      const int sl = slot >> 6, ln = slot & 63;
      const int b0 = g.by_dst.base[sl], w = (g.by_dst.base[sl + 1] - b0) >> 6;
      float acc = b0 + w * 64 <= res_cap ? sell_row_sum(lres + b0 + ln, w, term) : sell_row_sum(g.by_dst.arc + b0 + ln, w, term);
      const unsigned h = g.by_dst.row[slot];
      if (h != 0xffffffffu) {
        acc *= inv;
        cur[h] = acc;  // alpha(t,h) before the leaky term
        local += acc;
      }
    }
    const float sum = block_sum(local, red, kDenThreads / 64);
    if (tid == 0) asum[t] = sum;
    for (int h = tid; h < H; h += kDenThreads) {  // AlphaDash(t)
      const float a = cur[h] + leaky * sum * g.init[h];
      cur[h] = a;
      prev[h] = a;
    }
    prev_sum = sum;
    __syncthreads();
  }
  float local = 0.f;
  for (int h = tid; h < H; h += kDenThreads) local += prev[h];
  const float tot = block_sum(local, red, kDenThreads / 64);
  if (tid == 0) {
    logprob[s] = (double)logf(tot) + logcorr;
    asum[T] = tot;  // reuse: total of alpha_dash(T) (asum[T] itself is not needed by the backward pass)
  }
}

// Objective only (tdnnf_chain_objf): den_forward_kernel's recursion with nothing kept per frame -- no backward pass will read alpha or its
// sums, so the two state vectors it alternates between are all the state there is, and the only thing written is logprob[s].  The arithmetic
// is den_forward_kernel's, term by term, so the log-probability has its bits.
// LDS_STATE: both vectors in LDS behind the output row (P + 2 Hs floats); otherwise in `gstate`, 2 Hs floats per sequence.  The plain loop forms
// the frame's new vector in the second buffer as FAST does (den_forward_kernel's stages it in its global alpha row and reads it back).
// FAST needs LDS_STATE.
template <bool LDS_STATE, bool FAST = false>
__global__ __launch_bounds__(kDenThreads) void den_logprob_kernel(DenDev g, MatView y, int B, int T, float leaky, int Hs, double *logprob, float *gstate) {
  static_assert(LDS_STATE || !FAST, "den_logprob_kernel: the FAST loop keeps its vectors in LDS");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float red[kDenThreads / 64];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int H = g.H, P = g.P;
  float *x = smem;  // P
  float *prev = LDS_STATE ? smem + ((P + 3) & ~3) : gstate + (size_t)s * 2 * Hs;
  float *nxt = prev + Hs;  // the frame's new vector
  int sb0[kDenFastSlots], sw[kDenFastSlots];
  unsigned srow[kDenFastSlots];
  float hinit[kDenFastStates];
  if constexpr (FAST) {
#pragma unroll
    for (int k = 0; k < kDenFastSlots; k++) {
      const int slot = tid + k * kDenThreads;
      sb0[k] = 0;
      sw[k] = 0;
      srow[k] = 0xffffffffu;
      if (slot < g.by_dst.nslices * 64) {
        sb0[k] = g.by_dst.base[slot >> 6];
        sw[k] = (g.by_dst.base[(slot >> 6) + 1] - sb0[k]) >> 6;
        srow[k] = g.by_dst.row[slot];
      }
    }
#pragma unroll
    for (int i = 0; i < kDenFastStates; i++) hinit[i] = tid + i * kDenThreads < H ? g.init[tid + i * kDenThreads] : 0.f;
  }
  for (int h = tid; h < H; h += kDenThreads) prev[h] = g.init[h] + leaky * g.init_sum * g.init[h];  // AlphaFirstFrame + AlphaDash(0)
  float prev_sum = g.init_sum;
  double logcorr = 0.0;
  RowAhead ra;
  ra.load(y.data + (size_t)s * y.stride, P, tid);
  __syncthreads();
  for (int t = 1; t <= T; t++) {
#pragma unroll
    for (int i = 0; i < kDenRowRegs; i++)
      if (tid + i * kDenThreads < P) x[tid + i * kDenThreads] = exp_limited(ra.v[i]);
    for (int p = tid + kDenRowRegs * kDenThreads; p < P; p += kDenThreads) x[p] = exp_limited(y.data[(size_t)((t - 1) * B + s) * y.stride + p]);
    if (t < T) ra.load(y.data + (size_t)(t * B + s) * y.stride, P, tid);
    __syncthreads();
    const float inv = 1.0f / prev_sum;
    logcorr += (double)logf(prev_sum);
    float local = 0.f;
    auto term = [&](const uint2 a) { return prev[a.x & 0xffffu] * __uint_as_float(a.y) * x[a.x >> 16]; };
    if constexpr (FAST) {
      const int ln = tid & 63;
#pragma unroll
      for (int k = 0; k < kDenFastSlots; k++) {
        if (srow[k] == 0xffffffffu && sw[k] == 0) continue;
        float acc = sell_row_sum(g.by_dst.arc + sb0[k] + ln, sw[k], term);
        if (srow[k] != 0xffffffffu) {
          acc *= inv;
          nxt[srow[k]] = acc;  // alpha(t,h) before the leaky term
          local += acc;
        }
      }
    } else {
      for (int slot = tid; slot < g.by_dst.nslices * 64; slot += kDenThreads) {
        const int sl = slot >> 6, ln = slot & 63;
        const int b0 = g.by_dst.base[sl], w = (g.by_dst.base[sl + 1] - b0) >> 6;
        float acc = sell_row_sum(g.by_dst.arc + b0 + ln, w, term);
        const unsigned h = g.by_dst.row[slot];
        if (h != 0xffffffffu) {
          acc *= inv;
          nxt[h] = acc;
          local += acc;
        }
      }
    }
    const float sum = block_sum(local, red, kDenThreads / 64);  // (its barriers: prev is no longer read, every row of nxt is written)
    if constexpr (FAST) {
#pragma unroll
      for (int i = 0; i < kDenFastStates; i++) {  // AlphaDash(t)
        const int h = tid + i * kDenThreads;
        if (h < H) nxt[h] = nxt[h] + leaky * sum * hinit[i];
      }
    } else {
      for (int h = tid; h < H; h += kDenThreads) nxt[h] = nxt[h] + leaky * sum * g.init[h];
    }
    float *other = prev;
    prev = nxt;
    nxt = other;
    prev_sum = sum;
    __syncthreads();
  }
  float local = 0.f;
  for (int h = tid; h < H; h += kDenThreads) local += prev[h];
  const float tot = block_sum(local, red, kDenThreads / 64);
  if (tid == 0) logprob[s] = (double)logf(tot) + logcorr;
}

// Backward: deriv[t*B+s][p] = deriv_weight * gamma_den(t, p)   (overwrites the whole row)
template <bool LDS_STATE>
__global__ __launch_bounds__(kDenThreads) void den_backward_kernel(DenDev g, MatView y, int B, int T, float leaky,
                                                                   const float *alpha_all, const float *asum_all,
                                                                   int Hs, float deriv_weight, MatView deriv,
                                                                   float *gstate) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float red[kDenThreads / 64];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int H = g.H, P = g.P, P4 = (P + 3) & ~3, H4 = (H + 3) & ~3;
  float *x = smem;
  float *bnext = LDS_STATE ? smem + P4 : gstate + (size_t)s * 3 * Hs;
  float *bcur = LDS_STATE ? bnext + H4 : bnext + Hs;
  float *ad = LDS_STATE ? bcur + H4 : bcur + Hs;  // alpha_dash(t) * inv_asum(t)
  const float *alpha = alpha_all + (size_t)s * (T + 1) * Hs;
  const float *asum = asum_all + (size_t)s * (T + 1);

  {  // BetaDashLastFrame + Beta(T)
    const float bd = 1.0f / asum[T];
    const float lsum = g.init_sum * bd;
    for (int h = tid; h < H; h += kDenThreads) bnext[h] = bd + leaky * lsum;
  }
  RowAhead ra;
  ra.load(y.data + (size_t)((T - 1) * B + s) * y.stride, P, tid);
  __syncthreads();
  for (int t = T - 1; t >= 0; t--) {
    const float inv = 1.0f / asum[t];
#pragma unroll
    for (int i = 0; i < kDenRowRegs; i++)
      if (tid + i * kDenThreads < P) x[tid + i * kDenThreads] = exp_limited(ra.v[i]);
    for (int p = tid + kDenRowRegs * kDenThreads; p < P; p += kDenThreads) x[p] = exp_limited(y.data[(size_t)(t * B + s) * y.stride + p]);
    if (t > 0) ra.load(y.data + (size_t)((t - 1) * B + s) * y.stride, P, tid);
    for (int h = tid; h < H; h += kDenThreads) ad[h] = alpha[(size_t)t * Hs + h] * inv;
    __syncthreads();
    // beta_dash(t, i) = sum over out-arcs
    float local = 0.f;
    for (int slot = tid; slot < g.by_src.nslices * 64; slot += kDenThreads) {
      const int sl = slot >> 6, ln = slot & 63;
      const int b0 = g.by_src.base[sl], w = (g.by_src.base[sl + 1] - b0) >> 6;
      const uint2 *ap = g.by_src.arc + b0 + ln;
      const float acc0 = sell_row_sum(ap, w, [&](const uint2 a) { return __uint_as_float(a.y) * x[a.x >> 16] * bnext[a.x & 0xffffu]; });
      float acc = acc0;
      const unsigned h = g.by_src.row[slot];
      if (h != 0xffffffffu) {
        acc *= inv;
        bcur[h] = acc;
        local += g.init[h] * acc;
      }
    }
    // occupancies by pdf: gamma(t,p) = x[p] * sum_arcs prob * alpha_dash(t,src)/A(t) * beta(t+1,dst)
    float *dr = deriv.data + (size_t)(t * B + s) * deriv.stride;
    for (int slot = tid; slot < g.by_pdf.nslices * 64; slot += kDenThreads) {
      const int sl = slot >> 6, ln = slot & 63;
      const int b0 = g.by_pdf.base[sl], w = (g.by_pdf.base[sl + 1] - b0) >> 6;
      const uint2 *ap = g.by_pdf.arc + b0 + ln;
      // (summed in double: the long rows of the three tables, and nothing renormalises a frame's occupancies behind this kernel)
      const float acc0 = (float)sell_row_sum<double>(ap, w, [&](const uint2 a) { return __uint_as_float(a.y) * ad[a.x & 0xffffu] * bnext[a.x >> 16]; });
      float acc = acc0;
      const unsigned p = g.by_pdf.row[slot];
      if (p != 0xffffffffu) dr[p] = deriv_weight * acc * x[p];
    }
    const float ls = block_sum(local, red, kDenThreads / 64);  // also orders the reads of bnext above
    for (int h = tid; h < H; h += kDenThreads) bcur[h] += leaky * ls;  // Beta(t)
    float *tmp = bnext;
    bnext = bcur;
    bcur = tmp;
    __syncthreads();
  }
}

// The backward half in two kernels that do not wait for the forward one (persistent form, state vectors in LDS).  As in the wide
// form below, the backward recursion is linear and homogeneous in its last frame, so it can run SELF-NORMALISED beside the
// forward recursion:  b(T, h) = 1,  S(t) = sum_h init_h b(t, h),
//   b(t, h) = sum_arcs p x(t, pdf) (b(t+1, dst) / S(t+1) + leaky),
// every b(t) and S(t) kept (another (T+1) x Hs floats per sequence); the occupancies then need no dependence between frames:
//   gamma(t, p) = x(t, p) sum_arcs p alpha_dash(t, src) (b(t+1, dst) / S(t+1) + leaky) / Zd(t),   Zd(t) = sum_h alpha_dash(t, h) b(t, h)
// -- one workgroup per (frame, sequence).  128 x 500 frames, 4 000 states: 17.8 -> 11.6 ms stand-alone (10 000 states: 34.5 -> 27.9),
// which is what the component-level entry point gets.  The trainer, which runs the denominator beside the xent head on a stream
// of its own, keeps the one-kernel backward pass: there the further stream bought nothing at 1500 x 128 (133.8 -> 134.6 ms) and
// cost 7 ms at 150 x 64 (18.5 -> 25.7: with the weight-gradient stream that is a fifth stream in flight, and beyond four they
// share hardware queues -- the same cliff as one side stream per natural-gradient buffer set).
template <bool FAST = false>
__global__ __launch_bounds__(kDenThreads) void den_beta_kernel(DenDev g, MatView y, int B, int T, float leaky, float *b_all, float *S_all, int Hs,
                                                               const unsigned *only_if, int res_cap) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float red[kDenThreads / 64];
  if (only_if && *only_if == 0) return;
  const int s = blockIdx.x, tid = threadIdx.x;
  const int H = g.H, P = g.P, P4 = (P + 3) & ~3;
  float *x = smem;       // P: exp of the frame's output row
  float *bn = smem + P4;  // H: b(t+1, .) / S(t+1) + leaky
  float *nb = bn + ((H + 3) & ~3);  // FAST: the frame's raw sums (den_forward_kernel)
  uint2 *lres = reinterpret_cast<uint2 *>(bn + ((H + 3) & ~3) * (FAST ? 2 : 1));  // (den_forward_kernel: the table's first res_cap arcs)
  for (int i = tid; i < res_cap; i += kDenThreads) lres[i] = g.by_src.arc[i];
  int sb0[kDenFastSlots], sw[kDenFastSlots];
  unsigned srow[kDenFastSlots];
  float sinit[kDenFastSlots];
  if constexpr (FAST) {
#pragma unroll
    for (int k = 0; k < kDenFastSlots; k++) {
      const int slot = tid + k * kDenThreads;
      sb0[k] = 0;
      sw[k] = 0;
      srow[k] = 0xffffffffu;
      sinit[k] = 0.f;
      if (slot < g.by_src.nslices * 64) {
        sb0[k] = g.by_src.base[slot >> 6];
        sw[k] = (g.by_src.base[(slot >> 6) + 1] - sb0[k]) >> 6;
        srow[k] = g.by_src.row[slot];
        if (srow[k] != 0xffffffffu) sinit[k] = g.init[srow[k]];
      }
    }
  }
  float *brow = b_all + (size_t)s * (T + 1) * Hs;
  float *S = S_all + (size_t)s * (T + 1);
  for (int h = tid; h < H; h += kDenThreads) {
    brow[(size_t)T * Hs + h] = 1.0f;
    bn[h] = 1.0f / g.init_sum + leaky;
  }
  if (tid == 0) S[T] = g.init_sum;
  RowAhead ra;
  ra.load(y.data + (size_t)((T - 1) * B + s) * y.stride, P, tid);
  __syncthreads();
  for (int t = T - 1; t >= 0; t--) {
#pragma unroll
    for (int i = 0; i < kDenRowRegs; i++)
      if (tid + i * kDenThreads < P) x[tid + i * kDenThreads] = exp_limited(ra.v[i]);
    for (int p = tid + kDenRowRegs * kDenThreads; p < P; p += kDenThreads) x[p] = exp_limited(y.data[(size_t)(t * B + s) * y.stride + p]);
    if (t > 0) ra.load(y.data + (size_t)((t - 1) * B + s) * y.stride, P, tid);
    __syncthreads();
    float *bcur = brow + (size_t)t * Hs;
    float local = 0.f;
    auto term = [&](const uint2 a) { return __uint_as_float(a.y) * x[a.x >> 16] * bn[a.x & 0xffffu]; };
    if constexpr (FAST) {
      const int ln = tid & 63;
#pragma unroll
      for (int k = 0; k < kDenFastSlots; k++) {
        if (srow[k] == 0xffffffffu && sw[k] == 0) continue;
        const float acc = sb0[k] + sw[k] * 64 <= res_cap ? sell_row_sum(lres + sb0[k] + ln, sw[k], term) : sell_row_sum(g.by_src.arc + sb0[k] + ln, sw[k], term);
        if (srow[k] != 0xffffffffu) {
          nb[srow[k]] = acc;
          local += sinit[k] * acc;
        }
      }
      const float St = block_sum(local, red, kDenThreads / 64);  // (its barriers: bn is no longer read, every row of nb is written)
      if (tid == 0) S[t] = St;
      const float inv = 1.0f / St;
#pragma unroll
      for (int i = 0; i < kDenFastStates; i++) {
        const int h = tid + i * kDenThreads;
        if (h < H) {
          const float v = nb[h];
          bcur[h] = v;
          bn[h] = v * inv + leaky;
        }
      }
      __syncthreads();
      continue;
    }
    for (int slot = tid; slot < g.by_src.nslices * 64; slot += kDenThreads) {
      const int sl = slot >> 6, ln = slot & 63;
      const int b0 = g.by_src.base[sl], w = (g.by_src.base[sl + 1] - b0) >> 6;
      float acc = b0 + w * 64 <= res_cap ? sell_row_sum(lres + b0 + ln, w, term) : sell_row_sum(g.by_src.arc + b0 + ln, w, term);
      const unsigned h = g.by_src.row[slot];
      if (h != 0xffffffffu) {
        bcur[h] = acc;
        local += g.init[h] * acc;
      }
    }
    const float St = block_sum(local, red, kDenThreads / 64);  // (its barriers also order the reads of bn above)
    if (tid == 0) S[t] = St;
    const float inv = 1.0f / St;
    for (int h = tid; h < H; h += kDenThreads) bn[h] = bcur[h] * inv + leaky;  // (other threads' rows: visible after block_sum's barriers)
    __syncthreads();
  }
}

// Occupancies of one (frame, sequence): deriv[t*B+s][p] = deriv_weight * gamma_den(t, p) (overwrites the whole row)
constexpr int kGammaThreads = 512;
__global__ __launch_bounds__(kGammaThreads) void den_gamma_kernel(DenDev g, MatView y, int B, int T, float leaky, const float *alpha_all, const float *b_all,
                                                                  const float *S_all, int Hs, float deriv_weight, MatView deriv) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float red[kGammaThreads / 64];
  const int t = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
  const int H = g.H, P = g.P, P4 = (P + 3) & ~3, H4 = (H + 3) & ~3;
  float *x = smem, *ad = smem + P4, *bn = ad + H4;
  const float *alpha = alpha_all + ((size_t)s * (T + 1) + t) * Hs;     // alpha_dash(t, .)
  const float *bt = b_all + ((size_t)s * (T + 1) + t) * Hs, *bt1 = bt + Hs;
  const float inv = 1.0f / S_all[(size_t)s * (T + 1) + t + 1];
  const float *yr = y.data + (size_t)(t * B + s) * y.stride;
  for (int p = tid; p < P; p += kGammaThreads) x[p] = exp_limited(yr[p]);
  float local = 0.f;
  for (int h = tid; h < H; h += kGammaThreads) {
    const float a = alpha[h];
    ad[h] = a;
    bn[h] = bt1[h] * inv + leaky;
    local += a * bt[h];
  }
  const float Zd = block_sum(local, red, kGammaThreads / 64);  // (also the barrier before ad / bn / x are read)
  const float scale = deriv_weight / Zd;
  float *dr = deriv.data + (size_t)(t * B + s) * deriv.stride;
  // (the slice table and row ids of a thread's rows first, all at once: fetched row by row they sat, one trip to L2 each, in front of every row's arcs
  // -- twelve rows per thread at 6 034 pdfs, 33 us per block of which the arcs themselves are a third)
  constexpr int kRows = 12;
  const int nslot = g.by_pdf.nslices * 64, ln = tid & 63;
  auto term = [&](const uint2 a) { return __uint_as_float(a.y) * ad[a.x & 0xffffu] * bn[a.x >> 16]; };
  for (int s0 = tid; s0 < nslot; s0 += kRows * kGammaThreads) {
    int b0[kRows], w[kRows];
    unsigned row[kRows];
#pragma unroll
    for (int k = 0; k < kRows; k++) {
      const int slot = s0 + k * kGammaThreads;
      b0[k] = 0;
      w[k] = 0;
      row[k] = 0xffffffffu;
      if (slot < nslot) {
        b0[k] = g.by_pdf.base[slot >> 6];
        w[k] = (g.by_pdf.base[(slot >> 6) + 1] - b0[k]) >> 6;
        row[k] = g.by_pdf.row[slot];
      }
    }
#pragma unroll
    for (int k = 0; k < kRows; k++) {
      if (row[k] == 0xffffffffu) continue;
      const float acc = sell_row_sum(g.by_pdf.arc + b0[k] + ln, w[k], term);
      dr[row[k]] = scale * acc * x[row[k]];
    }
  }
}

// sell_row_sum for N sums over the same arcs, the term of arc a in sum n being pa(a, n) * pb(a, n): every arc is loaded once, and each sum gets
// den_gamma_kernel's bits.  That is sell_row_sum's order AND the instructions the compiler made of it there: rounded products and adds (its
// products come packed in pairs, v_pk_mul_f32, which leaves no add to fuse with) except the first term of the last batch, which it fuses into the
// sum (v_fmac_f32).  Contraction is off here and in the caller's factors (two sums side by side would otherwise become v_pk_fma_f32), and that one
// fused term is an explicit fmaf.
template <int N, class Fa, class Fb>
__device__ __forceinline__ void sell_row_sums(const uint2 *ap, int w, float (&acc)[N], Fa pa, Fb pb) {
#pragma clang fp contract(off)
#pragma unroll
  for (int n = 0; n < N; n++) acc[n] = 0.f;
  int j = 0;
  for (; j + 8 <= w; j += 8) {
    uint2 a[8];
#pragma unroll
    for (int u = 0; u < 8; u++) a[u] = ap[(j + u) * 64];
#pragma unroll
    for (int u = 0; u < 8; u++)
#pragma unroll
      for (int n = 0; n < N; n++) acc[n] += pa(a[u], n) * pb(a[u], n);
  }
  if (j + 4 <= w) {
    uint2 a[4];
#pragma unroll
    for (int u = 0; u < 4; u++) a[u] = ap[(j + u) * 64];
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
      for (int n = 0; n < N; n++) acc[n] += pa(a[u], n) * pb(a[u], n);
    j += 4;
  }
  if (j < w) {
    uint2 a[3];
#pragma unroll
    for (int u = 0; u < 3; u++) a[u] = ap[min(j + u, w - 1) * 64];
#pragma unroll
    for (int n = 0; n < N; n++) acc[n] = __builtin_fmaf(pa(a[0], n), pb(a[0], n), acc[n]);
#pragma unroll
    for (int u = 1; u < 3; u++)
#pragma unroll
      for (int n = 0; n < N; n++) acc[n] += (j + u < w) ? pa(a[u], n) * pb(a[u], n) : 0.f;
  }
}

// The occupancies of TWO consecutive frames of one sequence per 1024-thread workgroup (where both frames' vectors and output rows fit the LDS;
// option den_gamma_pairs = 1: den_gamma_kernel).  den_gamma_kernel streams the whole by-pdf arc table from L2 for every (frame, sequence) --
// 384 KB at 48 000 arcs, 3.5 ms of the pass alone at 4 000 states / 128 x 500 -- to use each arc once; here every arc loaded serves both
// frames.  A frame's output row is formed in LDS (scale * sum, in place of x = exp(y)) and written in one coalesced pass that reads y in the
// same order, instead of a scattered 4-byte store per row.  Same bits as den_gamma_kernel: each 512-thread half forms its frame's Zd with
// den_gamma_kernel's lanes and order, a row adds its arcs in SELL order as (prob * ad) * bn, and deriv = (scale * sum) * x.
constexpr int kGamma2Threads = 2 * kGammaThreads;
__global__ __launch_bounds__(kGamma2Threads) void den_gamma2_kernel(DenDev g, MatView y, int B, int T, float leaky, const float *alpha_all, const float *b_all,
                                                                    const float *S_all, int Hs, float deriv_weight, MatView deriv) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float red[kGamma2Threads / 64];
  const int t0 = 2 * blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
  const int H = g.H, P = g.P, P4 = (P + 3) & ~3, H4 = (H + 3) & ~3, L = 2 * H4 + P4;  // per frame: ad, bn, the output row
  const int nf = min(2, T - t0);  // (odd T: the last workgroup's second half forms frame t0 again and writes nothing)
  {
    const int f = tid / kGammaThreads, ht = tid % kGammaThreads, t = min(t0 + f, T - 1);
    float *ad = smem + f * L, *bn = ad + H4;
    const float *alpha = alpha_all + ((size_t)s * (T + 1) + t) * Hs;  // alpha_dash(t, .)
    const float *bt = b_all + ((size_t)s * (T + 1) + t) * Hs, *bt1 = bt + Hs;
    const float inv = 1.0f / S_all[(size_t)s * (T + 1) + t + 1];
    // (a thread's states in batches of eight, every load of a batch in flight at once: one at a time they were eight trips to HBM in a row; the
    // two fmaf are what den_gamma_kernel's compiled loop does, and states past H add exact zeros to a sum of non-negative terms)
    constexpr int kBatch = 8;
    float local = 0.f;
    for (int h0 = ht; h0 < H; h0 += kBatch * kGammaThreads) {
      float av[kBatch], bv[kBatch], b1v[kBatch];
#pragma unroll
      for (int i = 0; i < kBatch; i++) {
        const int h = h0 + i * kGammaThreads;
        av[i] = h < H ? alpha[h] : 0.f;
        bv[i] = h < H ? bt[h] : 0.f;
        b1v[i] = h < H ? bt1[h] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < kBatch; i++) {
        const int h = h0 + i * kGammaThreads;
        if (h < H) {
          ad[h] = av[i];
          bn[h] = __builtin_fmaf(b1v[i], inv, leaky);
        }
        local = __builtin_fmaf(av[i], bv[i], local);
      }
    }
    for (int o = 32; o > 0; o >>= 1) local += __shfl_xor(local, o, 64);  // (block_sum over this half's 8 waves)
    if ((tid & 63) == 0) red[tid >> 6] = local;
  }
  __syncthreads();
  float scale[2];
#pragma unroll
  for (int f = 0; f < 2; f++) {
    float Zd = 0.f;
    for (int w = 0; w < kGammaThreads / 64; w++) Zd += red[f * (kGammaThreads / 64) + w];
    scale[f] = deriv_weight / Zd;
  }
  constexpr int kRows = 8;
  const int nslot = g.by_pdf.nslices * 64, ln = tid & 63;
  auto pa = [&](const uint2 a, int f) {  // prob * ad(src); the term is (prob * ad) * bn(dst), as in den_gamma_kernel
#pragma clang fp contract(off)
    return __uint_as_float(a.y) * smem[f * L + (a.x & 0xffffu)];
  };
  auto pb = [&](const uint2 a, int f) { return smem[f * L + H4 + (a.x >> 16)]; };
  for (int s0 = tid; s0 < nslot; s0 += kRows * kGamma2Threads) {
    int b0[kRows], w[kRows];
    unsigned row[kRows];
#pragma unroll
    for (int k = 0; k < kRows; k++) {
      const int slot = s0 + k * kGamma2Threads;
      b0[k] = 0;
      w[k] = 0;
      row[k] = 0xffffffffu;
      if (slot < nslot) {
        b0[k] = g.by_pdf.base[slot >> 6];
        w[k] = (g.by_pdf.base[(slot >> 6) + 1] - b0[k]) >> 6;
        row[k] = g.by_pdf.row[slot];
      }
    }
#pragma unroll
    for (int k = 0; k < kRows; k++) {
      if (row[k] == 0xffffffffu) continue;
      float acc[2];
      sell_row_sums<2>(g.by_pdf.arc + b0[k] + ln, w[k], acc, pa, pb);
#pragma unroll
      for (int f = 0; f < 2; f++) smem[f * L + 2 * H4 + row[k]] = scale[f] * acc[f];
    }
  }
  __syncthreads();
  constexpr int kOut = 6;  // (both frames' y loads of a batch in flight at once)
  for (int p0 = tid; p0 < P; p0 += kOut * kGamma2Threads) {
    float yv[2][kOut];
#pragma unroll
    for (int f = 0; f < 2; f++)
#pragma unroll
      for (int i = 0; i < kOut; i++) {
        const int p = p0 + i * kGamma2Threads;
        yv[f][i] = f < nf && p < P ? y.data[(size_t)((t0 + f) * B + s) * y.stride + p] : 0.f;
      }
#pragma unroll
    for (int f = 0; f < 2; f++) {
      if (f >= nf) break;
      const float *o = smem + f * L + 2 * H4;
      float *dr = deriv.data + (size_t)((t0 + f) * B + s) * deriv.stride;
#pragma unroll
      for (int i = 0; i < kOut; i++) {
        const int p = p0 + i * kGamma2Threads;
        if (p < P) dr[p] = o[p] * exp_limited(yv[f][i]);
      }
    }
  }
}

}  // namespace
}  // namespace tdnnf
