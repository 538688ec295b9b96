// wgrad_kernels.h -- the weight-gradient kernels for gfx950 (MI355X, CDNA4); launched by wgrad.hip only.
//
// They replace the per-tap cuBLAS SGEMMs of TdnnDARTSV3Component::UpdateSimple
// (src/nnet3/nnet-tdnn-component.cc:452):
//   wgrad : G[o][i*Di+d] += lr * c_i * sum_rows dY[r][o] X_i[r][d]   (split over rows,
//           deterministic slab reduction)
// with the tiles, staging and arithmetic of the rows GEMM kernels (rows_gemm_kernels.h).
#pragma once
#include "common.h"
#include "gemm_dev.h"
#include "gemm_f32.h"

namespace tdnnf {
namespace {

// A = dY (k = row, m = output dim contiguous), B = X_tap (k = row, n = input dim contiguous).
template <int WM, int WN, int TM, int TN, int VEC, int TAG = 0>  // TAG: as for rows_gemm_kernel
__global__ __launch_bounds__(256) void wgrad_kernel(const WgradArgs p, int ntm, int ntn_tap, int rows_per_split,
                                                    float *partial) {
  constexpr int BK = 32;
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  constexpr int LDAS = BM + 4, LDBS = BN + 4;
  constexpr int A_TILE = BK * LDAS, B_TILE = BK * LDBS;
  constexpr int A_F4 = (BM * BK / 4 + 255) / 256, B_F4 = (BN * BK / 4 + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *As = smem, *Bs = smem + 2 * A_TILE;

  // Block -> (row split, tile, tap).  The taps of a component are row shifts of ONE matrix, so the blocks that differ only in the
  // tap stream the same slab of the big operand (X for the .linear components, dY for the .affine ones): they are given
  // neighbouring logical ids, and every XCD (workgroups are dealt to the eight XCDs round-robin) a contiguous run of logical ids,
  // so that a slab's second reader finds it in the L2 the first one filled instead of fetching it over the fabric again.
  const int tiles = ntm * (int)gridDim.x / ntm;  // = gridDim.x: ntm * taps launched * ntn_tap
  int bid = blockIdx.x, split = blockIdx.y;
  int tile_m, tile_n, tap;
  if (p.xcd_order) {
    const int nb = gridDim.x * gridDim.y, b = blockIdx.y * gridDim.x + blockIdx.x;
    const int q = nb / 8, r = nb % 8, xcd = b % 8, j = b / 8;
    const int L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
    const int ktaps = (int)gridDim.x / (ntm * ntn_tap);
    split = L / tiles;
    const int w = L % tiles;
    tap = w % ktaps;
    tile_m = (w / ktaps) % ntm;
    tile_n = (w / ktaps) / ntm;
  } else {
    tile_m = bid % ntm;
    tap = (bid / ntm) / ntn_tap;
    tile_n = (bid / ntm) % ntn_tap;
  }
  if (p.active) {  // compacted tap list: slots beyond the active count have nothing to do
    if (tap >= p.active[0]) return;
    tap = p.active[1 + tap];
  }
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int r_begin = split * rows_per_split;
  const int r_end = min(p.N, r_begin + rows_per_split);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave / WN, wn = wave % WN, li = lane & 31, lh = lane >> 5;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; a++)
#pragma unroll
    for (int b = 0; b < TN; b++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[a][b][r] = 0.f;

  const float cf = p.coef ? p.coef[tap] : 1.f;
  const float *Xb = p.X + (long long)p.row_offsets[tap] * p.ldx;
  const long long xrow = (long long)p.row_stride * p.ldx;

  float4 ra[A_F4], rb[B_F4];
  // Fast path (whole K-step inside the split, 16-byte accesses, Do and Di multiples of 4): per-thread source pointers
  // set up once; a column group that is out of range reads 16 zero bytes with step 0 instead of branching, which
  // keeps the steady-state loop a single basic block (accumulators stay in AGPRs).
  const bool fast_ok = VEC == 4 && p.Do % 4 == 0 && p.Di % 4 == 0;
  const float *aptr[A_F4], *bptr[B_F4];
  long long astep[A_F4], bstep[B_F4];
  {
    const float *zero = reinterpret_cast<const float *>(&g_zero4);
#pragma unroll
    for (int j = 0; j < A_F4; j++) {
      const int idx = t + 256 * j, kr = idx / (BM / 4), m = m0 + (idx % (BM / 4)) * 4;
      const bool v = (BM * BK / 4 % 256 == 0 || idx < BM * BK / 4) && m < p.Do;
      aptr[j] = v ? p.dY + (long long)kr * p.lddy + m : zero;
      astep[j] = v ? p.lddy : 0;
    }
#pragma unroll
    for (int j = 0; j < B_F4; j++) {
      const int idx = t + 256 * j, kr = idx / (BN / 4), n = n0 + (idx % (BN / 4)) * 4;
      const bool v = (BN * BK / 4 % 256 == 0 || idx < BN * BK / 4) && n < p.Di;
      bptr[j] = v ? Xb + (long long)kr * xrow + n : zero;
      bstep[j] = v ? xrow : 0;
    }
  }
  auto load_tile = [&](int r0) {
    if (fast_ok && r0 + BK <= r_end) {
#pragma unroll
      for (int j = 0; j < A_F4; j++) ra[j] = *reinterpret_cast<const float4 *>(aptr[j] + (long long)r0 * astep[j]);
#pragma unroll
      for (int j = 0; j < B_F4; j++) rb[j] = *reinterpret_cast<const float4 *>(bptr[j] + (long long)r0 * bstep[j]);
      return;
    }
#pragma unroll
    for (int j = 0; j < A_F4; j++) {
      const int idx = t + 256 * j;
      const int kr = idx / (BM / 4), m = m0 + (idx % (BM / 4)) * 4;
      const bool rv = (BM * BK / 4 % 256 == 0 || idx < BM * BK / 4) && r0 + kr < r_end;
      const float *ptr = p.dY + (long long)(r0 + kr) * p.lddy + m;
      ra[j] = ld4(ptr, rv && m < p.Do, rv && m + 1 < p.Do, rv && m + 2 < p.Do, rv && m + 3 < p.Do, VEC == 4);
    }
#pragma unroll
    for (int j = 0; j < B_F4; j++) {
      const int idx = t + 256 * j;
      const int kr = idx / (BN / 4), n = n0 + (idx % (BN / 4)) * 4;
      const bool rv = (BN * BK / 4 % 256 == 0 || idx < BN * BK / 4) && r0 + kr < r_end;
      const float *ptr = Xb + (long long)(r0 + kr) * xrow + n;
      rb[j] = ld4(ptr, rv && n < p.Di, rv && n + 1 < p.Di, rv && n + 2 < p.Di, rv && n + 3 < p.Di, VEC == 4);
    }
  };
  auto store_tile = [&](int buf) {
    float *as = As + buf * A_TILE, *bs = Bs + buf * B_TILE;
#pragma unroll
    for (int j = 0; j < A_F4; j++) {
      const int idx = t + 256 * j;
      if (BM * BK / 4 % 256 == 0 || idx < BM * BK / 4)
        *reinterpret_cast<float4 *>(as + (idx / (BM / 4)) * LDAS + (idx % (BM / 4)) * 4) = ra[j];
    }
#pragma unroll
    for (int j = 0; j < B_F4; j++) {
      const int idx = t + 256 * j;
      if (BN * BK / 4 % 256 == 0 || idx < BN * BK / 4)
        *reinterpret_cast<float4 *>(bs + (idx / (BN / 4)) * LDBS + (idx % (BN / 4)) * 4) = rb[j];
    }
  };
  auto compute = [&](int buf) {
    const float *as = As + buf * A_TILE + lh * LDAS + wm * TM * 32 + li;
    const float *bs = Bs + buf * B_TILE + lh * LDBS + wn * TN * 32 + li;
    // fragments of k-pair k2 + 1 are requested before the MFMAs of k-pair k2 are issued (two register sets), so the
    // LDS latency hides behind TM * TN MFMAs instead of stalling every other one
    float a[2][TM], b[2][TN];
#pragma unroll
    for (int i = 0; i < TM; i++) a[0][i] = as[i * 32];
#pragma unroll
    for (int i = 0; i < TN; i++) b[0][i] = bs[i * 32];
#pragma unroll
    for (int k2 = 0; k2 < BK / 2; k2++) {
      const int cur = k2 & 1, nxt = cur ^ 1;
      if (k2 + 1 < BK / 2) {
#pragma unroll
        for (int i = 0; i < TM; i++) a[nxt][i] = as[(2 * k2 + 2) * LDAS + i * 32];
#pragma unroll
        for (int i = 0; i < TN; i++) b[nxt][i] = bs[(2 * k2 + 2) * LDBS + i * 32];
      }
#pragma unroll
      for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cur][i], b[cur][j], acc[i][j], 0, 0, 0);
    }
  };

  // partial slab [split][Do][K*Di]
  float *P = partial + (long long)split * p.Do * (p.K * p.Di);
  if (cf == 0.f) return;  // skipped tap: the reduce kernel does not read its slab
  if (r_begin >= r_end) {  // (cannot happen with the host's split plan; keep the slab defined anyway)
    for (int e = t; e < BM * BN; e += 256) {
      const int m = m0 + e / BN, n = n0 + e % BN;
      if (m < p.Do && n < p.Di) P[(long long)m * (p.K * p.Di) + tap * p.Di + n] = 0.f;
    }
    return;
  }
  // straight-line prologue / loop / epilogue: with the loop under a condition the register allocator kept the 64-80
  // accumulators in VGPRs across the back edge and copied them to AGPRs every K-step (288 registers, one wave per SIMD)
  load_tile(r_begin);
  store_tile(0);
  __syncthreads();
  {
    int buf = 0;
    for (int r0 = r_begin;; r0 += BK) {
      const bool more = r0 + BK < r_end;
      if (more) load_tile(r0 + BK);
      compute(buf);
      if (!more) break;
      store_tile(buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }
  }
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TN; j++) {
      const int n = n0 + (wn * TN + j) * 32 + li;
      if (n >= p.Di) continue;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int m = m0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (m < p.Do) P[(long long)m * (p.K * p.Di) + tap * p.Di + n] = acc[i][j][r];
      }
    }
}

// The weight gradient in split-bf16 arithmetic (see rows_gemm_x3_kernel).  Both operands are reduced over rows, so a
// fragment needs 8 consecutive ROWS of one column: every thread loads one column of 8 rows (dword loads, consecutive
// lanes on consecutive columns: coalesced), splits it and writes one 16-byte [column][k] piece per plane.
template <int WM, int WN, int TM, int TN, int NP, int D, int TAG = 0>
__global__ __launch_bounds__(256, 2) void wgrad_x3_kernel(const WgradArgs p, int ntm, int ntn_tap, int rows_per_split, float *partial) {
  constexpr int BK = NP == 2 ? 32 : 16, LDH = BK + 8;  // three planes: half the K-step, the same LDS budget
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  constexpr int A_IT = (BM * BK / 8 + 255) / 256, B_IT = (BN * BK / 8 + 255) / 256;  // (column, 8-row group) items per thread
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __bf16 *As = reinterpret_cast<__bf16 *>(smem);       // [2 buffers][NP planes][BM][LDH]
  __bf16 *Bs = As + 2 * NP * BM * LDH;                 // [2 buffers][NP planes][BN][LDH]

  int bid = blockIdx.x;
  const int tile_m = bid % ntm;
  int tap = (bid / ntm) / ntn_tap;
  const int tile_n = (bid / ntm) % ntn_tap;
  if (p.active) {
    if (tap >= p.active[0]) return;
    tap = p.active[1 + tap];
  }
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int split = blockIdx.y;
  const int r_begin = split * rows_per_split;
  const int r_end = min(p.N, r_begin + rows_per_split);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave / WN, wn = wave % WN, li = lane & 31, lh = lane >> 5;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; a++)
#pragma unroll
    for (int b = 0; b < TN; b++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[a][b][r] = 0.f;

  const float cf = p.coef ? p.coef[tap] : 1.f;
  const float *Xb = p.X + (long long)p.row_offsets[tap] * p.ldx;
  const long long xrow = (long long)p.row_stride * p.ldx;

  float ra[D][A_IT][8], rb[D][B_IT][8];  // D staged K-steps (see rows_gemm_x3_kernel)
  // per-item source: column pointer at row 0 of the item's 8-row group; an out-of-range column reads zeros (step 0)
  const float *aptr[A_IT], *bptr[B_IT];
  long long astep[A_IT], bstep[B_IT];
  int akg[A_IT], bkg[B_IT];
  {
    const float *zero = reinterpret_cast<const float *>(&g_zero4);
#pragma unroll
    for (int j = 0; j < A_IT; j++) {
      const int item = t + 256 * j, col = item % BM, kg = item / BM;
      const bool v = (BM * BK / 8 % 256 == 0 || item < BM * BK / 8) && m0 + col < p.Do;
      akg[j] = kg;
      aptr[j] = v ? p.dY + (long long)(kg * 8) * p.lddy + m0 + col : zero;
      astep[j] = v ? p.lddy : 0;
    }
#pragma unroll
    for (int j = 0; j < B_IT; j++) {
      const int item = t + 256 * j, col = item % BN, kg = item / BN;
      const bool v = (BN * BK / 8 % 256 == 0 || item < BN * BK / 8) && n0 + col < p.Di;
      bkg[j] = kg;
      bptr[j] = v ? Xb + (long long)(kg * 8) * xrow + n0 + col : zero;
      bstep[j] = v ? xrow : 0;
    }
  }
  // whole K-step inside the split: unconditional loads (a branch-free steady state, see rows_gemm_x3_kernel)
  auto load_fast = [&](float (&ra)[A_IT][8], float (&rb)[B_IT][8], int r0) {
#pragma unroll
    for (int j = 0; j < A_IT; j++) {
      const float *q = aptr[j] + (long long)r0 * astep[j];
#pragma unroll
      for (int i = 0; i < 8; i++) ra[j][i] = q[(long long)i * astep[j]];
    }
#pragma unroll
    for (int j = 0; j < B_IT; j++) {
      const float *q = bptr[j] + (long long)r0 * bstep[j];
#pragma unroll
      for (int i = 0; i < 8; i++) rb[j][i] = q[(long long)i * bstep[j]];
    }
  };
  auto load_ragged = [&](float (&ra)[A_IT][8], float (&rb)[B_IT][8], int r0) {  // the split's last, partial K-step
#pragma unroll
    for (int j = 0; j < A_IT; j++) {
      const float *q = aptr[j] + (long long)r0 * astep[j];
#pragma unroll
      for (int i = 0; i < 8; i++) ra[j][i] = r0 + akg[j] * 8 + i < r_end ? q[(long long)i * astep[j]] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < B_IT; j++) {
      const float *q = bptr[j] + (long long)r0 * bstep[j];
#pragma unroll
      for (int i = 0; i < 8; i++) rb[j][i] = r0 + bkg[j] * 8 + i < r_end ? q[(long long)i * bstep[j]] : 0.f;
    }
  };
  auto split8 = [](const float *x, bf16x8 (&pl)[NP]) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
      float r = x[i];
#pragma unroll
      for (int q = 0; q < NP; q++) {
        const __bf16 h = (__bf16)r;
        pl[q][i] = h;
        r -= (float)h;
      }
    }
  };
  auto store_tile = [&](const float (&ra)[A_IT][8], const float (&rb)[B_IT][8], int buf) {
    __bf16 *ah = As + buf * NP * BM * LDH, *bh = Bs + buf * NP * BN * LDH;
#pragma unroll
    for (int j = 0; j < A_IT; j++) {
      const int item = t + 256 * j;
      if (BM * BK / 8 % 256 == 0 || item < BM * BK / 8) {
        bf16x8 pl[NP];
        split8(ra[j], pl);
        const int o = (item % BM) * LDH + (item / BM) * 8;
#pragma unroll
        for (int q = 0; q < NP; q++) *reinterpret_cast<bf16x8 *>(ah + q * BM * LDH + o) = pl[q];
      }
    }
#pragma unroll
    for (int j = 0; j < B_IT; j++) {
      const int item = t + 256 * j;
      if (BN * BK / 8 % 256 == 0 || item < BN * BK / 8) {
        bf16x8 pl[NP];
        split8(rb[j], pl);
        const int o = (item % BN) * LDH + (item / BN) * 8;
#pragma unroll
        for (int q = 0; q < NP; q++) *reinterpret_cast<bf16x8 *>(bh + q * BN * LDH + o) = pl[q];
      }
    }
  };
  auto compute = [&](int buf) {
    const __bf16 *ah = As + buf * NP * BM * LDH + (wm * TM * 32 + li) * LDH + lh * 8;
    const __bf16 *bh = Bs + buf * NP * BN * LDH + (wn * TN * 32 + li) * LDH + lh * 8;
#pragma unroll
    for (int c = 0; c < BK / 16; c++) {
      bf16x8 a[NP][TM], b[NP][TN];
#pragma unroll
      for (int q = 0; q < NP; q++) {
#pragma unroll
        for (int i = 0; i < TM; i++) a[q][i] = *reinterpret_cast<const bf16x8 *>(ah + q * BM * LDH + i * 32 * LDH + c * 16);
#pragma unroll
        for (int i = 0; i < TN; i++) b[q][i] = *reinterpret_cast<const bf16x8 *>(bh + q * BN * LDH + i * 32 * LDH + c * 16);
      }
#pragma unroll
      for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++) {
#pragma unroll
          for (int d = NP - 1; d >= 0; d--)
#pragma unroll
            for (int q = 0; q <= d; q++)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[q][i], b[d - q][j], acc[i][j], 0, 0, 0);
        }
    }
  };

  float *P = partial + (long long)split * p.Do * (p.K * p.Di);
  if (cf == 0.f) return;
  if (r_begin >= r_end) {
    for (int e = t; e < BM * BN; e += 256) {
      const int m = m0 + e / BN, n = n0 + e % BN;
      if (m < p.Do && n < p.Di) P[(long long)m * (p.K * p.Di) + tap * p.Di + n] = 0.f;
    }
    return;
  }
  {
    bool have[D];
    int rnext = r_begin;  // first row of the next K-step to stage
    int buf = 0;
    static_for<D>([&](auto uc) {
      constexpr int u = decltype(uc)::value;
      have[u] = rnext + BK <= r_end;
      if (have[u]) {
        load_fast(ra[u], rb[u], rnext);
        rnext += BK;
      }
    });
    if (have[0]) {
      store_tile(ra[0], rb[0], 0);
      __syncthreads();
      if (have[D - 1]) {
        // steady state: LDS buffer `buf` holds the step staged in slot u, slots u+1 .. u+D-1 the next D - 1 steps
        bool run = true;
        while (run) {
          static_for<D>([&](auto uc) {
            constexpr int u = decltype(uc)::value;
            if (!run) return;
            if (rnext + BK > r_end) {  // no full step left to stage: drain
              static_for<D - 1>([&](auto jc) {
                constexpr int nx = (u + 1 + decltype(jc)::value) % D;
                compute(buf);
                store_tile(ra[nx], rb[nx], buf ^ 1);
                __syncthreads();
                buf ^= 1;
              });
              compute(buf);
              run = false;
              return;
            }
            load_fast(ra[u], rb[u], rnext);
            rnext += BK;
            compute(buf);
            constexpr int nx = (u + 1) % D;
            store_tile(ra[nx], rb[nx], buf ^ 1);
            __syncthreads();
            buf ^= 1;
          });
        }
      } else {  // fewer than D full steps
        bool run = true;
        static_for<D>([&](auto uc) {
          constexpr int u = decltype(uc)::value;
          if (!run) return;
          compute(buf);
          if constexpr (u + 1 >= D) {
            run = false;
          } else {
            if (!have[u + 1]) {
              run = false;
              return;
            }
            store_tile(ra[u + 1], rb[u + 1], buf ^ 1);
            __syncthreads();
            buf ^= 1;
          }
        });
      }
    }
    if (rnext < r_end) {  // ragged end; buffer buf ^ 1 is free (last read before the last barrier)
      load_ragged(ra[0], rb[0], rnext);
      store_tile(ra[0], rb[0], buf ^ 1);
      __syncthreads();
      compute(buf ^ 1);
    }
  }
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TN; j++) {
      const int n = n0 + (wn * TN + j) * 32 + li;
      if (n >= p.Di) continue;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int m = m0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (m < p.Do) P[(long long)m * (p.K * p.Di) + tap * p.Di + n] = acc[i][j][r];
      }
    }
}

// G[o][c] (+)= scale * coef[tap(c)] * sum_split partial[split][o][c]
__global__ void wgrad_reduce_kernel(const float *partial, int splits, int Do, int KDi, int Di, const float *coef,
                                    float scale, float *G, long long ldg, int accumulate, const float *ds1 = nullptr, const float *ds2 = nullptr) {
  if (ds1) scale *= ds1[1] * ds2[1];  // plane operands: the reciprocals of the scales they were split with
  const long long total = (long long)Do * KDi;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const int o = (int)(e / KDi), c = (int)(e % KDi);
    float s = 0.f;
#pragma unroll 4
    for (int sp = 0; sp < splits; sp++) s += partial[(long long)sp * total + e];
    const float cf = coef ? coef[c / Di] : 1.f;
    if (cf == 0.f) continue;  // skipped tap: its slab may not have been written
    float *g = G + (long long)o * ldg + c;
    const float v = scale * cf * s;
    *g = accumulate ? *g + v : v;
  }
}

// The same for small outputs (the R x R products of the natural-gradient statistics: one tile, hundreds of row
// splits): 16 split groups per element so the serial chain is splits/16 loads long.
__global__ __launch_bounds__(256) void wgrad_reduce_small_kernel(const float *partial, int splits, int Do, int KDi, int Di, const float *coef,
                                                                 float scale, float *G, long long ldg, int accumulate) {
  __shared__ float red[16][17];
  const int el = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const long long total = (long long)Do * KDi, e = blockIdx.x * 16LL + el;
  float s = 0.f;
  if (e < total)
    for (int sp = grp; sp < splits; sp += 16) s += partial[(long long)sp * total + e];
  red[grp][el] = s;
  __syncthreads();
  if (grp != 0 || e >= total) return;
  s = 0.f;
#pragma unroll
  for (int g = 0; g < 16; g++) s += red[g][el];
  const int o = (int)(e / KDi), c = (int)(e % KDi);
  const float cf = coef ? coef[c / Di] : 1.f;
  if (cf == 0.f) return;
  float *g = G + (long long)o * ldg + c;
  const float v = scale * cf * s;
  *g = accumulate ? *g + v : v;
}

// column sums of dY in two deterministic stages: partial[chunk][col] then bias_acc[col] += scale*sum
__global__ void colsum_partial_kernel(const float *Y, long long ld, int rows, int cols, int rows_per_chunk,
                                      float *partial) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  const int r0 = blockIdx.y * rows_per_chunk, r1 = min(rows, r0 + rows_per_chunk);
  if (col >= cols) return;
  float s = 0.f;
  for (int r = r0; r < r1; r++) s += Y[(long long)r * ld + col];
  partial[(long long)blockIdx.y * cols + col] = s;
}
__global__ void colsum_final_kernel(const float *partial, int chunks, int cols, float scale, float *acc) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= cols) return;
  float s = 0.f;
  for (int c = 0; c < chunks; c++) s += partial[(long long)c * cols + col];
  acc[col] += scale * s;
}

}  // namespace
}  // namespace tdnnf
