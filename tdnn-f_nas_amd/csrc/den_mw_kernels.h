// den_mw_kernels.h -- the denominator's two recursions with several workgroups per sequence.  Launched by chain_den.hip only.
#pragma once
#include "den_dev.h"

namespace tdnnf {
namespace {

// ---- The two recursions with SEVERAL workgroups per sequence (few sequences: the 8-GPU shard of a minibatch, the recipes' own egs).
// One workgroup per sequence walks T dependent frames at ~15 us each -- 384 KB of arcs from L2 per frame on one CU, and the fixed work of
// a frame -- while the other CUs have nothing to do.  Here G workgroups share a sequence: slice k of the SELL table belongs to workgroup
// k % G (every workgroup gets the same mix of row degrees), its arcs stay in LDS for the whole kernel, and per frame a workgroup
//   publishes the new values of its rows (exchange buffer in slot order, double-buffered by frame parity: agent-scope stores, every
//   wave's vmcnt(0), workgroup barrier, one agent-scope add to the sequence's counter),
//   waits until the counter shows all G slices of the frame (one lane polls; bounded: on a time-out it raises the abort word, which
//   every poll also reads, and the host reports an error instead of hanging), and
//   reads the whole vector back (agent-scope loads) into LDS, where the frame's normaliser is summed.
// MI355X_MICROARCH.md, inter-workgroup visibility: stores and loads of the handed-off bytes all sc1, the signal behind every storing
// wave's wait and a barrier, the loads behind the poll and a barrier.  A buffer of parity q is rewritten for frame t + 2 only after the
// counter has reached G (t + 1), i.e. after every workgroup has published frame t + 1, which it does after reading frame t.
// The workgroups of a sequence sit on one XCD when the sequence count is a multiple of 8 (blocks b and b + 8 share an XCD).
struct MwCtl {
  unsigned long long *ctr;  // [2 * B]: forward counters, then backward counters
  unsigned *abort_flag;
  float *xf, *xb;           // [B][2][NSp] exchange buffers of the forward / backward recursion
  int NSp;
};
constexpr unsigned kMwSpinLimit = 1u << 22;  // polls of ~0.5 us: seconds -- a launch that cannot make progress ends, it does not hang

__device__ __forceinline__ void mw_block_of(int b, int B, int G, int *s, int *gi) {
  if (B % 8 == 0) {
    const int x = b & 7, j = b >> 3;
    *s = (j / G) * 8 + x;
    *gi = j % G;
  } else {
    *s = b / G;
    *gi = b % G;
  }
}
// publish: all of this workgroup's stores are issued; wait, barrier, one add.
__device__ __forceinline__ void mw_publish(unsigned long long *ctr) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_fetch_add(ctr, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// consume: wait for `target` adds (one lane polls, the others wait at the barrier).  Returns false on abort.
__device__ __forceinline__ bool mw_wait(unsigned long long *ctr, unsigned *abort_flag, unsigned target, unsigned *lds_flag) {
  if (threadIdx.x == 0) {
    unsigned spins = 0, ab = 0;
    while (true) {
      const unsigned long long v = __hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      ab = __hip_atomic_load(abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((unsigned)v >= target || ab) break;
      if (++spins > kMwSpinLimit) {
        __hip_atomic_store(abort_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ab = 1;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    *lds_flag = ab;
  }
  __syncthreads();
  return *lds_flag == 0;
}

// dir 0: alpha recursion over by_dst (as den_forward_kernel<true>); dir 1: the self-normalised beta recursion over by_src (den_beta_kernel)
template <int DIR>
__global__ __launch_bounds__(kDenThreads) void den_mw_kernel(DenDev g, MwCtl ctl, int G, MatView y, int B, int T, float leaky, float *vec_all, float *sum_all,
                                                             int Hs, double *logprob) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float red[kDenThreads / 64];
  __shared__ unsigned flag;
  __shared__ int loff[64 + 1];  // LDS offsets (arc entries) of the slices this workgroup owns
  const tdnnf_den_graph::Sell &tab = DIR == 0 ? g.by_dst : g.by_src;
  int s, gi;
  mw_block_of(blockIdx.x, B, G, &s, &gi);
  const int tid = threadIdx.x;
  const int H = g.H, P = g.P, P4 = (P + 3) & ~3, H4 = (H + 3) & ~3, ns = tab.nslices, NSp = ctl.NSp;
  float *x = smem;            // P: exp of the frame's output row
  float *cur = smem + P4;     // H: the previous frame's vector, by state (forward: alpha_dash(t-1); backward: b(t+1)/S(t+1) + leaky)
  uint2 *arcs = reinterpret_cast<uint2 *>(cur + H4);
  unsigned long long *ctr = ctl.ctr + (DIR == 0 ? s : B + s);
  float *xch = (DIR == 0 ? ctl.xf : ctl.xb) + (size_t)s * 2 * NSp;
  float *vec = vec_all + (size_t)s * (T + 1) * Hs;
  float *sums = sum_all + (size_t)s * (T + 1);
  const int nown = ns > gi ? (ns - gi + G - 1) / G : 0;  // slices gi, gi + G, ...
  if (tid == 0) {
    int o = 0;
    for (int i = 0; i < nown; i++) {
      loff[i] = o;
      const int k = gi + i * G;
      o += tab.base[k + 1] - tab.base[k];
    }
    loff[nown] = o;
  }
  __syncthreads();
  for (int i = 0; i < nown; i++) {
    const int k = gi + i * G, b0 = tab.base[k], n = tab.base[k + 1] - b0;
    for (int e = tid; e < n; e += kDenThreads) arcs[loff[i] + e] = tab.arc[b0 + e];
  }
  // the share of the final arrays this workgroup writes: states [h0, h1)
  const int h0 = (int)((long long)H * gi / G), h1 = (int)((long long)H * (gi + 1) / G);
  float prev_sum = g.init_sum;
  double logcorr = 0.0;
  if (DIR == 0) {  // AlphaFirstFrame + AlphaDash(0)
    for (int h = tid; h < H; h += kDenThreads) {
      const float a = g.init[h] + leaky * g.init_sum * g.init[h];
      cur[h] = a;
      if (h >= h0 && h < h1) vec[h] = a;
    }
    if (gi == 0 && tid == 0) sums[0] = g.init_sum;
  } else {  // b(T, .) = 1, S(T) = sum init
    for (int h = tid; h < H; h += kDenThreads) {
      cur[h] = 1.0f / g.init_sum + leaky;
      if (h >= h0 && h < h1) vec[(size_t)T * Hs + h] = 1.0f;
    }
    if (gi == 0 && tid == 0) sums[T] = g.init_sum;
  }
  __syncthreads();
  // the output row of a frame is requested (into registers) before the exchange of the frame before it and turned into x behind it:
  // its trip to memory runs under the wait for the other workgroups
  constexpr int kRowRegs = 8, kRowThreads = kDenThreads - 64;  // waves 1-15: P <= 8 * 960 (checked on the host)
  float yv[kRowRegs];
  const int rt = tid - 64;
  auto request_row = [&](int step) {
    const int yrow = DIR == 0 ? step - 1 : T - step;
    const float *yr = y.data + (size_t)(yrow * B + s) * y.stride;
    if (rt >= 0) {
#pragma unroll
      for (int i = 0; i < kRowRegs; i++) yv[i] = rt + i * kRowThreads < P ? yr[rt + i * kRowThreads] : 0.f;
    }
  };
  auto row_to_x = [&]() {
    if (rt >= 0) {
#pragma unroll
      for (int i = 0; i < kRowRegs; i++)
        if (rt + i * kRowThreads < P) x[rt + i * kRowThreads] = exp_limited(yv[i]);
    }
  };
  float *stage = reinterpret_cast<float *>(arcs + loff[nown]);  // nown * 64: this workgroup's new values, for 16-byte stores
  request_row(1);
  row_to_x();
  __syncthreads();
  for (int step = 1; step <= T; step++) {
    const int t = DIR == 0 ? step : T - step;  // the frame whose vector is formed
    const float inv = 1.0f / prev_sum;
    if (DIR == 0) logcorr += (double)logf(prev_sum);
    float *xw = xch + (size_t)(step & 1) * NSp;
    for (int q = tid; q < nown * 64; q += kDenThreads) {
      const int i = q >> 6, ln = q & 63;
      const int w = (loff[i + 1] - loff[i]) >> 6;
      const uint2 *ap = arcs + loff[i] + ln;
      const float acc0 = sell_row_sum(ap, w, [&](const uint2 a) { return cur[a.x & 0xffffu] * __uint_as_float(a.y) * x[a.x >> 16]; });
      float acc = acc0;
      if (DIR == 0) acc *= inv;
      stage[q] = acc;  // (a padding slot: 0)
    }
    __syncthreads();
    for (int q = tid; q < nown * 16; q += kDenThreads) {  // 16 bytes per store, agent scope
      const int i = q >> 4, c = q & 15, k = gi + i * G;
      const f32x4 v = *reinterpret_cast<const f32x4 *>(stage + i * 64 + c * 4);
      asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(xw + k * 64 + c * 4), "v"(v) : "memory");
    }
    mw_publish(ctr);
    if (step < T) request_row(step + 1);  // (behind the signal; not by the polling wave, whose polls would queue behind these loads)
    if (!mw_wait(ctr, ctl.abort_flag, (unsigned)(G * step), &flag)) return;
    // the whole vector of this frame, slot order -> by state; its normaliser
    float local = 0.f;
    for (int q4 = tid; q4 < ns * 16; q4 += kDenThreads) {
      f32x4 v;
      asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(xw + q4 * 4) : "memory");
      const uint4 hh = *reinterpret_cast<const uint4 *>(tab.row + q4 * 4);
      const unsigned hs[4] = {hh.x, hh.y, hh.z, hh.w};
#pragma unroll
      for (int e = 0; e < 4; e++) {
        if (hs[e] != 0xffffffffu) {
          cur[hs[e]] = v[e];
          local += DIR == 0 ? v[e] : g.init[hs[e]] * v[e];
        }
      }
    }
    const float sum = block_sum(local, red, kDenThreads / 64);  // (its barriers order the writes of cur above before the reads below)
    if (gi == 0 && tid == 0) sums[t] = sum;
    if (DIR == 0) {
      for (int h = tid; h < H; h += kDenThreads) {  // AlphaDash(t)
        const float a = cur[h] + leaky * sum * g.init[h];
        cur[h] = a;
        if (h >= h0 && h < h1) vec[(size_t)t * Hs + h] = a;
      }
    } else {
      const float is = 1.0f / sum;
      for (int h = tid; h < H; h += kDenThreads) {
        const float v = cur[h];
        if (h >= h0 && h < h1) vec[(size_t)t * Hs + h] = v;  // b(t, h), as den_beta_kernel keeps it
        cur[h] = v * is + leaky;
      }
    }
    if (step < T) row_to_x();
    prev_sum = sum;
    __syncthreads();
  }
  if (DIR == 0) {
    float local = 0.f;
    for (int h = tid; h < H; h += kDenThreads) local += cur[h];
    const float tot = block_sum(local, red, kDenThreads / 64);
    if (gi == 0 && tid == 0) {
      logprob[s] = (double)logf(tot) + logcorr;
      sums[T] = tot;  // (as den_forward_kernel: the total of alpha_dash(T))
    }
  }
}

// a multi-workgroup launch that gave up (mw_wait's time-out: its workgroups were not co-resident, e.g. under a CU mask or beside another
// process): the one-workgroup kernels launched behind it redo both recursions (they look at the same word), and the host learns of it
// through a counter in pinned memory -- chain_den() reports it once and stops using the multi-workgroup form in this process
__global__ void den_mw_check_kernel(const unsigned *abort_flag, unsigned *host_fallbacks) {
  if (*abort_flag != 0 && threadIdx.x == 0) __hip_atomic_fetch_add(host_fallbacks, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace
}  // namespace tdnnf
