// den_wide_kernels.h -- the denominator's wide form: one launch per frame over all sequences.  Launched by chain_den.hip only.
#pragma once
#include "den_dev.h"

namespace tdnnf {
namespace {

// ---------------------------------------------------------------------------------------------- denominator, wide form
// The persistent kernels above give a sequence one workgroup and keep its state vectors in LDS: right while they fit (up to
// ~10 000 states), a crawl beyond (30 000 states / 360 000 arcs: every arc is a 4-byte gather from L2, 580 ms per
// minibatch).  The wide form runs the recursion one frame per launch over ALL sequences with the SEQUENCE as the fastest
// index of every array (Kaldi's own choice, for the same reason), in GROUPS of SG sequences (32; 16 for minibatches of <= 16):
//   alpha[t][group][state][SG],  x[t][group][pdf][SG]          (SG = 32: one whole 128-byte line per state, line-aligned)
//  * a wave is SG sequences x 64/SG rows (states / pdfs).  The arcs of its rows are not fetched arc by arc: one coalesced
//    16-byte load per lane brings 64 arcs (4 arc positions of the wave's 16 rows) as (state | pdf << 16, p, p init_src), and
//    each lane group picks the arc of its row out of the holder's registers with ds_bpermute (the LDS crossbar, no memory).
//    Per arc step that leaves the two gathers the recursion cannot do without (alpha_src, x_pdf): the leaky-HMM term
//    alpha_dash = alpha + leaky A init_src costs no third one because p init_src travels in the arc.
//  * a workgroup serves ONE group: group = blockIdx.x % num_groups.  Workgroups go to the eight XCDs round-robin, so an XCD
//    only ever touches the frame slices of its own group(s) -- at 128 sequences and SG 32: 30 000 states x 128 bytes = 3.8 MB
//    of alpha + 0.8 MB of x against a 4 MB L2 (measured hit rate 77 %, 3.4 M L2 requests per launch; SG 16 fits better, 89 %
//    of 6.3 M, and is slower: L2 requests are per line, and a 64-byte run is half a line).  Runs that straddle a line cost a
//    second request each: every array of the wide form is 128-byte aligned.  The arc table streams past with non-temporal loads.
//  * the normaliser A(t-1, s) = sum_h alpha(t-1, h, s) is NOT a launch of its own between two frames: every workgroup of frame
//    t starts by summing the previous launch's partial sums for its group's sequences (fixed order, float4 loads all in
//    flight at once), so a frame is ONE launch forward and one backward.
// Measured (30 000 states / 360 000 arcs, 128 x 500 frames, tools/den_bench.py): 56 ms for the whole objective, from 105 ms with
// one 256-byte run per state and arc-by-arc loads; a recursion launch takes 48 us alone, 55 us beside the other direction's.
constexpr int kWideBatch = 8;   // arc steps whose picks and gathers are issued together (a multiple of 4)
constexpr int kWideSlices = 2;  // SELL slices (of 64 rows) per 256-thread block of the recursions: a wave takes 16 rows of each

struct WideDims {
  int B, NG, SG;  // sequences, groups, sequences per group (16 or 32; NG * SG >= B)
};

typedef unsigned uv4 __attribute__((ext_vector_type(4)));

// xT[t][g][p][sl] = exp(clamp(y[t*B + g*SG + sl][p])): per frame a B x P -> P x B transpose through LDS
__global__ __launch_bounds__(256) void den_wide_prep_kernel(MatView y, WideDims d, int P, float *xT) {
  __shared__ float tile[64][65];
  const int t = blockIdx.z, p0 = blockIdx.x * 64, s0 = blockIdx.y * 64, tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int i = ty; i < 64; i += 4) {
    const int sq = s0 + i, p = p0 + tx;
    tile[i][tx] = (sq < d.B && p < P) ? exp_limited(y.data[(size_t)(t * d.B + sq) * y.stride + p]) : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 64; i += 4) {
    const int p = p0 + i, sq = s0 + tx;
    if (p < P && sq < d.NG * d.SG) xT[(((size_t)t * d.NG + sq / d.SG) * P + p) * d.SG + sq % d.SG] = tile[tx][i];
  }
}
// deriv[t*B + s][p] = dT[t][g][p][sl]
__global__ __launch_bounds__(256) void den_wide_unprep_kernel(const float *dT, WideDims d, int P, MatView deriv) {
  __shared__ float tile[64][65];
  const int t = blockIdx.z, p0 = blockIdx.x * 64, s0 = blockIdx.y * 64, tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int i = ty; i < 64; i += 4) {
    const int p = p0 + i, sq = s0 + tx;
    tile[i][tx] = (p < P && sq < d.B) ? dT[(((size_t)t * d.NG + sq / d.SG) * P + p) * d.SG + sq % d.SG] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 64; i += 4) {
    const int sq = s0 + i, p = p0 + tx;
    if (sq < d.B && p < P) deriv.data[(size_t)(t * d.B + sq) * deriv.stride + p] = tile[tx][i];
  }
}

// frame 0 of alpha (before the leaky term) / frame T of b: v[g][h][sl] = init_h or 1; norm[s] = init_sum
__global__ __launch_bounds__(256) void den_wide_init_kernel(DenDev g, WideDims d, int Hs, bool ones, float *v, float *norm) {
  const long long total = (long long)d.NG * Hs * d.SG;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {  // (grid_for caps the grid)
    const int h = (int)((e / d.SG) % Hs);
    v[e] = h < g.H ? (ones ? 1.0f : g.init[h]) : 0.f;
  }
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < d.B; e += gridDim.x * 256LL) norm[e] = g.init_sum;
}

// where a workgroup of the recursion kernels stands: its group, its block of slices, its lane's sequence and row lane
template <int SG>
struct WideLane {
  static constexpr int RL = 64 / SG;  // rows side by side in a wave
  static constexpr int IT = 16 / RL;  // passes over a wave's 16 rows
  int grp, blk, sl, rl, sq, wave, lane;
  bool on;
  __device__ WideLane(const WideDims &d, int g, int b) {
    lane = threadIdx.x & 63;
    wave = threadIdx.x >> 6;
    grp = g;
    blk = b;
    sl = lane % SG;
    rl = lane / SG;
    sq = grp * SG + sl;
    on = sq < d.B;
  }
};
// Normaliser of the previous launch for this lane's sequence: the sum of the group's `nblk` partial sums, 256/SG threads per
// sequence and four of them per load, then the threads' sums in fixed order (the same number in every workgroup); stored by
// the first workgroup of a group.  part[group][sequence][npad], npad = nblk rounded up to 4 with the tail zeroed: the sums of one
// sequence are contiguous, and every thread has all its loads (<= 8 float4 for up to 1 024 partial sums at SG 32) in flight at
// once -- the partial sums were written by the previous launch, possibly through another XCD's L2, so each load is a trip to
// memory, and a chain of them was most of a frame's time.
__device__ __forceinline__ int wide_npad(int nblk) { return (nblk + 3) & ~3; }
template <int SG>
__device__ __forceinline__ float wide_norm(const float *part, int nblk, float *norm_out, float *red, const WideLane<SG> &L) {
  constexpr int NQ = 256 / SG;
  const int q = threadIdx.x / SG, nch = wide_npad(nblk) >> 2;
  const float4 *pp = (const float4 *)(part + ((size_t)L.grp * SG + L.sl) * wide_npad(nblk));
  float v = 0.f;
  for (int c0 = q; c0 < nch; c0 += 8 * NQ) {
    float4 f[8];
#pragma unroll
    for (int u = 0; u < 8; u++) f[u] = c0 + u * NQ < nch ? pp[c0 + u * NQ] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int u = 0; u < 8; u++) v += (f[u].x + f[u].y) + (f[u].z + f[u].w);
  }
  red[q * SG + L.sl] = v;
  __syncthreads();
  float tot = 0.f;
#pragma unroll
  for (int i = 0; i < NQ; i++) tot += red[i * SG + L.sl];
  __syncthreads();  // red is used again for the block's own partial
  if (L.blk == 0 && q == 0 && L.on) norm_out[L.sq] = tot;
  return L.on ? tot : 1.0f;
}
// sum of `v` over the block's rows for each sequence of the group -> part[grp][sl][blk] (padding sequences: 0)
template <int SG>
__device__ __forceinline__ void wide_store_partial(float v, float *red, float *part, int nblk, const WideLane<SG> &L) {
#pragma unroll
  for (int o = SG; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  if (L.rl == 0) red[L.wave * SG + L.sl] = v;
  __syncthreads();
  if (threadIdx.x < SG) {
    float *row = part + ((size_t)L.grp * SG + L.sl) * wide_npad(nblk);
    row[L.blk] = (red[L.sl] + red[SG + L.sl]) + (red[2 * SG + L.sl] + red[3 * SG + L.sl]);
    if (L.blk == nblk - 1)
      for (int k = nblk; k < wide_npad(nblk); k++) row[k] = 0.f;
  }
}
// One load for 4 consecutive arc positions of a wave's 16 rows: lane l holds arc (position jb + l/16, row l%16 of the 16)
__device__ __forceinline__ uv4 wide_load_arcs(const uv4 *ap, int jb, int w, int lane) {
  const int j = jb + (lane >> 4);
  uv4 a = {0u, 0u, 0u, 0u};
  if (j < w) a = __builtin_nontemporal_load(ap + (size_t)j * 64);
  return a;
}

// The arcs of one SELL slice for this wave's 16 rows.  Every arc step needs the arc's (key, p, p init_src) and two gathered
// values: t1[(key & 0xffff) * SG + sl] and t2[(key >> 16) * SG + sl].  kWideBatch steps at a time: all their picks and gathers are
// issued before the first product is formed, and the load of the next four arc positions goes out BEHIND the gathers -- loads
// complete in order, so an arc load (a trip to memory) issued ahead of them would hold every gather's data back.
// MODE 0 forward:  acc += t2 p t1,  acl += t2 p init_src           (t1 = alpha(t-1), t2 = x(t-1))
// MODE 1 backward: acc += p t2 t1,  acl += p t2                    (t1 = b(t+1),     t2 = x(t))
// MODE 2 occupancy: acc += (t1 p + c0 p init_src) (t2 c1 + c2)      (t1 = alpha(t),   t2 = b(t+1); c0 = leaky A, c1 = 1/S, c2 = leaky)
template <int SG, int MODE>
__device__ __forceinline__ void wide_slice(const tdnnf_den_graph::Sell &T, int slice, const float *t1, const float *t2, const WideLane<SG> &L, float c0, float c1,
                                           float c2, float *acc, float *acl) {
  using WL = WideLane<SG>;
  const int b0 = T.base[slice], w = (T.base[slice + 1] - b0) >> 6;
  const uv4 *ap = (const uv4 *)T.arc4 + b0 + L.wave * 16 + (L.lane & 15);
  uv4 a = wide_load_arcs(ap, 0, w, L.lane);
  constexpr int BS = kWideBatch, NB = WL::IT * 4 / BS;  // arc steps per batch, batches per four arc positions
  for (int jb = 0; jb < w; jb += 4) {
    uv4 an = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int h = 0; h < NB; h++) {
      float g1[BS], g2[BS], pr[BS], iq[BS];
#pragma unroll
      for (int k = 0; k < BS; k++) {
        const int e = h * BS + k, row4 = ((e / 4) * WL::RL + L.rl) * 4 + (e % 4) * 64;  // step e: row pass e/4, arc position e%4
        const unsigned key = (unsigned)__builtin_amdgcn_ds_bpermute(row4, (int)a.x);
        pr[k] = __int_as_float(__builtin_amdgcn_ds_bpermute(row4, (int)a.y));
        iq[k] = MODE != 1 ? __int_as_float(__builtin_amdgcn_ds_bpermute(row4, (int)a.z)) : 0.f;
        g1[k] = t1[(key & 0xffffu) * SG + L.sl];
        g2[k] = t2[(key >> 16) * SG + L.sl];
      }
      if (h == NB - 1) an = wide_load_arcs(ap, jb + 4, w, L.lane);  // zeros past the end
#pragma unroll
      for (int k = 0; k < BS; k++) {
        const int it = (h * BS + k) / 4;
        if (MODE == 0) {
          acc[it] += g2[k] * pr[k] * g1[k];
          acl[it] += g2[k] * iq[k];
        } else if (MODE == 1) {
          const float px = pr[k] * g2[k];
          acc[it] += px * g1[k];
          acl[it] += px;
        } else {
          acc[it] += (g1[k] * pr[k] + c0 * iq[k]) * (g2[k] * c1 + c2);
        }
      }
      // keep the next batch's picks and loads behind this batch's arithmetic (4 BS live values each): the arc registers are
      // "redefined" here and the batch's sums "used"
      asm volatile("" : "+v"(a.x), "+v"(a.y), "+v"(a.z)::"memory");
#pragma unroll
      for (int it = h * BS / 4; it < (h + 1) * BS / 4; it++) {
        asm volatile("" : "+v"(acc[it]));
        if (MODE != 2) asm volatile("" : "+v"(acl[it]));
      }
    }
    a = an;
  }
}

// alpha(t, h, s) = 1/A(t-1, s) sum_arcs alpha_dash(t-1, src, s) p x(t-1, pdf, s)
//               = (1/A) sum_arcs alpha(t-1, src, s) p x + leaky sum_arcs p init_src x        (alpha_dash = alpha + leaky A init).
// part_prev: launch t-1's partial sums of A(t-1) (null at t = 1: A(0) is in asum[0] already); nsl: slices per block
// TWO_FRAMES (tdnnf_chain_objf: objective only, no backward pass will read the other T - 1): alphaT holds two frames, frame t in alphaT[t & 1];
// the normalisers keep their (T + 1) x B array, den_wide_total_kernel sums their logarithms
template <int SG, bool TWO_FRAMES = false>
__global__ __launch_bounds__(256) void den_wide_fwd_kernel(DenDev g, WideDims d, int t, float leaky, const float *xT, float *alphaT, float *asum, int Hs,
                                                           const float *part_prev, int nblk, int nsl, float *part) {
  using WL = WideLane<SG>;
  __shared__ float red[256];
  const WL L(d, blockIdx.x % d.NG, blockIdx.x / d.NG);
  const size_t frame = (size_t)d.NG * Hs * SG;
  const float *prev = alphaT + (size_t)(TWO_FRAMES ? (t - 1) & 1 : t - 1) * frame + (size_t)L.grp * Hs * SG;  // uniform; lanes add (state * SG + sl)
  float *cur = alphaT + (size_t)(TWO_FRAMES ? t & 1 : t) * frame + (size_t)L.grp * Hs * SG;
  const float *x = xT + ((size_t)(t - 1) * d.NG + L.grp) * g.P * SG;
  const int s0 = L.blk * nsl, s1 = min(s0 + nsl, g.by_dst.nslices);
  const float Aprev = part_prev ? wide_norm<SG>(part_prev, nblk, asum + (size_t)(t - 1) * d.B, red, L) : (L.on ? asum[(size_t)(t - 1) * d.B + L.sq] : 1.f);
  const float inv = 1.0f / Aprev;
  float total = 0.f;
  for (int slice = s0; slice < s1; slice++) {
    float acc[WL::IT], acl[WL::IT];
#pragma unroll
    for (int it = 0; it < WL::IT; it++) acc[it] = acl[it] = 0.f;
    wide_slice<SG, 0>(g.by_dst, slice, prev, x, L, 0.f, 0.f, 0.f, acc, acl);
#pragma unroll
    for (int it = 0; it < WL::IT; it++) {
      const unsigned h = g.by_dst.row[slice * 64 + L.wave * 16 + it * WL::RL + L.rl];
      if (h != 0xffffffffu && L.on) {
        const float v = acc[it] * inv + leaky * acl[it];
        cur[h * SG + L.sl] = v;
        total += v;
      }
    }
  }
  wide_store_partial<SG>(total, red, part, nblk, L);
}

// out[s] = sum over the nblk partial rows, in the order wide_norm takes them (after the last frame of a recursion)
template <int SG>
__global__ __launch_bounds__(256) void den_wide_sum_kernel(const float *part, int nblk, WideDims d, float *out) {
  __shared__ float red[256];
  const WideLane<SG> L(d, blockIdx.x, 0);
  wide_norm<SG>(part, nblk, out, red, L);
}

// tot(s) = sum_h alpha_dash(T, h, s) = A(T, s) (1 + leaky init_sum); log-prob of the sequence
__global__ __launch_bounds__(256) void den_wide_total_kernel(DenDev g, int B, int T, float leaky, const float *asum, double *logprob) {
  const int sq = blockIdx.x * 256 + threadIdx.x;
  if (sq >= B) return;
  const float tt = asum[(size_t)T * B + sq] * (1.0f + leaky * g.init_sum);
  double lc = 0.0;
  for (int t = 0; t < T; t++) lc += (double)logf(asum[(size_t)t * B + sq]);
  logprob[sq] = (double)logf(tt) + lc;
}

// The backward recursion does not wait for the forward one: it runs SELF-NORMALISED on a stream of its own, beside it.
// beta_dash is linear and homogeneous in its last frame, so with b(T, h) = 1, S(t) = sum_h init_h b(t, h) and
//   b(t, h, s) = sum_arcs p x(t, pdf, s) (b(t+1, dst, s) / S(t+1, s) + leaky)
// the true beta_dash(t) is a per-(frame, sequence) multiple of b(t) (the leaky term of the normalised vector is the constant
// `leaky`: sum_h init_h b/S = 1).  The multiple never has to be formed: the occupancies of a frame sum to one, so
//   gamma(t, p, s) = x(t, p, s) sum_arcs p alpha_dash(t, src, s) (b(t+1, dst, s) / S(t+1, s) + leaky) / Zd(t, s),
//   Zd(t, s) = sum_h alpha_dash(t, h, s) b(t, h, s)        (= the sum over p of the numerators, by the recursion above),
// which needs alpha (kept for every frame anyway) and b for every frame (another (T+1) x H x B floats: 7.7 GB at 30 000 states,
// 128 x 500 frames -- what 288 GB are for) and leaves the occupancy pass with no dependence between frames: ONE launch over
// all of them instead of one per frame.

// b(t) from b(t+1) (bnextT) and S(t+1) = (1/S) sum_arcs p x b(t+1, dst) + leaky sum_arcs p x; partials of S(t) = sum_h init_h b(t, h, s).
// part_prev: the partial sums of launch t+1 (null at t = T-1: S(T) is in S already)
template <int SG>
__global__ __launch_bounds__(256) void den_wide_beta_kernel(DenDev g, WideDims d, int t, float leaky, const float *xT, const float *bnextT, float *S, int Hs,
                                                            float *bcurT, const float *part_prev, int nblk, int nsl, float *part) {
  using WL = WideLane<SG>;
  __shared__ float red[256];
  const WL L(d, blockIdx.x % d.NG, blockIdx.x / d.NG);
  const float *bnext = bnextT + (size_t)L.grp * Hs * SG;
  float *bcur = bcurT + (size_t)L.grp * Hs * SG;
  const float *x = xT + ((size_t)t * d.NG + L.grp) * g.P * SG;
  const int s0 = L.blk * nsl, s1 = min(s0 + nsl, g.by_src.nslices);
  const float Snext = part_prev ? wide_norm<SG>(part_prev, nblk, S + (size_t)(t + 1) * d.B, red, L) : (L.on ? S[(size_t)(t + 1) * d.B + L.sq] : 1.f);
  const float inv = 1.0f / Snext;
  float total = 0.f;
  for (int slice = s0; slice < s1; slice++) {
    float acc[WL::IT], acl[WL::IT];
#pragma unroll
    for (int it = 0; it < WL::IT; it++) acc[it] = acl[it] = 0.f;
    wide_slice<SG, 1>(g.by_src, slice, bnext, x, L, 0.f, 0.f, 0.f, acc, acl);
#pragma unroll
    for (int it = 0; it < WL::IT; it++) {
      const unsigned h = g.by_src.row[slice * 64 + L.wave * 16 + it * WL::RL + L.rl];
      if (h != 0xffffffffu && L.on) {
        const float v = acc[it] * inv + leaky * acl[it];
        bcur[h * SG + L.sl] = v;
        total += g.init[h] * v;
      }
    }
  }
  wide_store_partial<SG>(total, red, part, nblk, L);
}

// Zd(t, s) = sum_h (alpha(t, h, s) + leaky A(t, s) init_h) b(t, h, s) for every frame: block (t, group), 256/SG threads per
// sequence stride the states
template <int SG>
__global__ __launch_bounds__(256) void den_wide_dot_kernel(DenDev g, WideDims d, float leaky, const float *alphaT, const float *asum, int Hs, const float *bT,
                                                           float *Zd) {
  __shared__ double red[256];
  const int t = blockIdx.x, grp = blockIdx.y, sl = threadIdx.x % SG, hl = threadIdx.x / SG, sq = grp * SG + sl;
  const size_t off = ((size_t)t * d.NG + grp) * Hs * SG + sl;
  const float *alpha = alphaT + off, *b = bT + off;
  double acc = 0.0;
  if (sq < d.B) {
    const float lka = leaky * asum[(size_t)t * d.B + sq];
    for (int h = hl; h < g.H; h += 256 / SG) acc += (double)((alpha[(size_t)h * SG] + lka * g.init[h]) * b[(size_t)h * SG]);
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  if (hl == 0 && sq < d.B) {
    double tot = 0.0;
    for (int q = 0; q < 256 / SG; q++) tot += red[q * SG + sl];
    Zd[(size_t)t * d.B + sq] = (float)tot;
  }
}

// x(t, p, s) <- deriv_weight gamma_den(t, p, s)  (in place), every frame in one launch: blockIdx.y = t, one SELL slice per
// block (x fastest: the resident waves stay within a frame or two, whose alpha and b slices an XCD's L2 can hold)
template <int SG>
__global__ __launch_bounds__(256) void den_wide_gamma_kernel(DenDev g, WideDims d, float leaky, float *xT, const float *alphaT, const float *asum, int Hs,
                                                             const float *bT, const float *S, const float *Zd, float deriv_weight) {
  using WL = WideLane<SG>;
  const WL L(d, blockIdx.x % d.NG, blockIdx.x / d.NG);
  const int t = blockIdx.y, slice = L.blk;
  const size_t frame = (size_t)d.NG * Hs * SG;
  const float *alpha = alphaT + (size_t)t * frame + (size_t)L.grp * Hs * SG, *bnext = bT + (size_t)(t + 1) * frame + (size_t)L.grp * Hs * SG;
  float *x = xT + ((size_t)t * d.NG + L.grp) * g.P * SG;
  float lka = 0.f, inv = 0.f, scale = 0.f;
  if (L.on) {
    lka = leaky * asum[(size_t)t * d.B + L.sq];
    inv = 1.0f / S[(size_t)(t + 1) * d.B + L.sq];
    scale = deriv_weight / Zd[(size_t)t * d.B + L.sq];
  }
  float acc[WL::IT];
#pragma unroll
  for (int it = 0; it < WL::IT; it++) acc[it] = 0.f;
  wide_slice<SG, 2>(g.by_pdf, slice, alpha, bnext, L, lka, inv, leaky, acc, nullptr);
#pragma unroll
  for (int it = 0; it < WL::IT; it++) {
    const unsigned p = g.by_pdf.row[slice * 64 + L.wave * 16 + it * WL::RL + L.rl];
    if (p != 0xffffffffu && L.on) x[p * SG + L.sl] *= scale * acc[it];
  }
}

}  // namespace
}  // namespace tdnnf
