// rows_gemm_kernels.h -- the rows GEMM kernels for gfx950 (MI355X, CDNA4); launched by rows_gemm.hip only.
//
// These replace the per-tap cuBLAS SGEMMs the reference issues from
// TdnnDARTSV3Component::Propagate / Backprop
// (src/nnet3/nnet-tdnn-component.cc:302-324, :378-411) and the
// AffineComponent / LinearComponent GEMMs (nnet-simple-component.cc:1235-1279).
//
// Arithmetic: v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate; bit-for-bit an fmaf
// chain, so parity with the reference's fp32 BaseFloat path is limited only by
// summation order).  One launch covers ALL taps of a layer:
//   rows_gemm : C[m][n] (+)= sum_taps c_i * A_i[m][:] . B_i[:][n]   (fwd and bwd-data,
//               bwd-data in gather form so overlapping taps need no atomics)
// Tiles: 4 waves / 256 threads, each wave owns TM x TN blocks of 32x32 accumulators;
// A/B tiles are staged global -> registers -> LDS (double buffered, one barrier per
// K-step); LDS rows are padded by 4 floats so the ds_read_b128 fragment reads are
// bank-conflict free (stride 36 / 20 dwords).
#pragma once
#include "common.h"
#include "gemm_dev.h"
#include "gemm_f32.h"

namespace tdnnf {
namespace {

// ------------------------------------------------------------------------ rows_gemm
// TAG only gives the launches of the natural-gradient statistics (ProfClassOverride(3)) their own kernel symbol, so
// that per-kernel profiler summaries keep them apart from the TDNN-F GEMMs; the code is identical.
// (the body of a block: block `bx` of the `gx` blocks that work on `p` -- the whole grid of a plain launch, one task's share of a grouped one)
// The inference epilogue of RowsGemmArgs (col_scale / col_offset / post_add / row_map) for a float4 of row m: pre = bias (or
// zero), addv = the addend.  Only rows_gemm_post_kernel instantiates rows_gemm_block with POST: every other kernel compiles the
// code it had before this stage existed.
__device__ __forceinline__ void post_store4(const RowsGemmArgs &p, int m, int n, float4 v, float4 pre, float4 addv) {
  v.x += pre.x; v.y += pre.y; v.z += pre.z; v.w += pre.w;
  if (!p.post_add) { v.x += p.add_scale * addv.x; v.y += p.add_scale * addv.y; v.z += p.add_scale * addv.z; v.w += p.add_scale * addv.w; }
  if (p.relu) { v.x = floor_keep_nan(v.x, 0.f); v.y = floor_keep_nan(v.y, 0.f); v.z = floor_keep_nan(v.z, 0.f); v.w = floor_keep_nan(v.w, 0.f); }
  const float4 sc = p.col_scale ? *reinterpret_cast<const float4 *>(p.col_scale + n) : make_float4(1.f, 1.f, 1.f, 1.f);
  const float4 of = p.col_offset ? *reinterpret_cast<const float4 *>(p.col_offset + n) : make_float4(0.f, 0.f, 0.f, 0.f);
  const float as = p.post_add ? p.add_scale : 0.f;
  v.x = sc.x * v.x + of.x + as * addv.x;
  v.y = sc.y * v.y + of.y + as * addv.y;
  v.z = sc.z * v.z + of.z + as * addv.z;
  v.w = sc.w * v.w + of.w + as * addv.w;
  const int mo = p.row_map ? p.row_map[m] : m;
  if (mo >= 0) *reinterpret_cast<float4 *>(p.C + (long long)mo * p.ldc + n) = v;
}
// the same for one element (tile edges, C rows without 16-byte alignment)
__device__ __forceinline__ void post_store1(const RowsGemmArgs &p, int m, int n, float x) {
  if (p.init_mode == 1) x += p.bias[n];
  const float a = (p.add && m >= p.add_lo && m < p.add_hi) ? p.add[(long long)(m - p.add_lo) * p.ldadd + n] : 0.f;
  if (!p.post_add) x += p.add_scale * a;
  if (p.relu) x = floor_keep_nan(x, 0.f);
  x = (p.col_scale ? p.col_scale[n] : 1.f) * x + (p.col_offset ? p.col_offset[n] : 0.f) + (p.post_add ? p.add_scale * a : 0.f);
  const int mo = p.row_map ? p.row_map[m] : m;
  if (mo >= 0) p.C[(long long)mo * p.ldc + n] = x;
}

template <int WM, int WN, int TM, int TN, int BK, bool B_KC, int VEC, bool POST = false>
__device__ __forceinline__ void rows_gemm_block(const RowsGemmArgs &p, int ntm, int ntn, int bx, int gx) {
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  constexpr int LDAS = BK + 4;
  constexpr int LDBS = B_KC ? BK + 4 : BN + 4;
  constexpr int A_TILE = BM * LDAS;
  constexpr int B_TILE = B_KC ? BN * LDBS : BK * LDBS;
  constexpr int A_F4 = (BM * BK / 4 + 255) / 256;
  constexpr int B_F4 = (BN * BK / 4 + 255) / 256;
  constexpr int KF4 = BK / 4;  // float4 per k-row of a k-contiguous tile
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *As = smem;               // [2][A_TILE]
  float *Bs = smem + 2 * A_TILE;  // [2][B_TILE]

  // XCD-aware tile order: blocks b and b+8 share an XCD (round-robin dispatch), so give each
  // XCD a contiguous run of logical tile ids; within it tile_n varies fastest so the blocks
  // that re-read the same A rows (and the taps' neighbouring rows) hit the same L2.
  const int nblk = ntm * ntn;
  int bid = bx;
  {
    const int q = nblk / 8, r = nblk % 8, xcd = bid % 8, j = bid / 8;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
  }
  int sp = 0;
  if (p.ksplit > 1) {  // split-K launch: consecutive block ids share a tile
    sp = bx % p.ksplit;
    bid = bx / p.ksplit;
  }
  const long long k_begin = (long long)sp * p.kchunk, k_end = p.ksplit > 1 ? k_begin + p.kchunk : (1LL << 60);
  const int tile_m = bid / ntn, tile_n = bid % ntn;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int li = lane & 31, lh = lane >> 5;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; a++)
#pragma unroll
    for (int b = 0; b < TN; b++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[a][b][r] = 0.f;

  // ---- K iterator over (segment, chunk), skipping zero-coefficient segments
  // (a split-K block only visits the part of each segment inside its [k_begin, k_end) slice)
  // (alt_seg_order: odd row tiles visit the segments in reverse.  The taps of a TDNN-F layer are row shifts of ONE matrix by a tile's worth
  // of rows, so row block i is the tap-0 operand of tile i and the tap-(-1) operand of tile i + 1: with every tile going tap by tap in the
  // same order the two reads are half a launch apart and both come from HBM -- PMC traffic 2.07 x the algorithmic bytes for the 160-wide
  // class in rounds 2-4; in alternating order both consumers of a row block read it in the same phase, at the same K step, on one XCD)
  const bool rev_seg = p.alt_seg_order && (tile_m & 1);
  int seg = -1, sgi = 0, kc = 0, klen = 0;  // seg: position in this tile's visiting order; sgi: the segment's index in p.seg
  long long seg_kstart = 0, seg_knext = 0;
  float cf = 1.f;
  auto next_seg = [&]() {
    for (++seg; seg < p.nseg; ++seg) {
      sgi = rev_seg ? p.nseg - 1 - seg : seg;
      seg_kstart = seg_knext;
      seg_knext += p.seg[sgi].klen;
      cf = p.coef ? p.coef[sgi] : 1.f;
      const long long lo = k_begin > seg_kstart ? k_begin - seg_kstart : 0;
      const long long hi = k_end < seg_knext ? k_end - seg_kstart : p.seg[sgi].klen;
      if (cf != 0.f && hi > lo) {
        kc = (int)lo;
        klen = (int)hi;
        return;
      }
    }
    kc = 0;
    klen = 0;
  };
  next_seg();

  float4 ra[A_F4], rb[B_F4];
  // The tap coefficient (and the sum of squares of p.sumsq) is applied when a staged tile goes to LDS, not when it is
  // loaded: anything that touches ra/rb right after the loads would wait for them in front of the MFMAs they are
  // supposed to overlap with.
  float cf_tile = 1.f;  // coefficient of the segment the tile in ra/rb was loaded from
  float ssq = 0.f;      // p.sumsq: running sum of (coef * a)^2 over everything this thread stages
  auto add_ssq = [&]() {
    // (plain v_fmac_f32 from inline assembly: written as a sum of products the compiler packs it into v_pk_mul_f32 / v_pk_add_f32, which
    // beside MFMAs cost several times their plain forms -- 622 against 482 us for the pass with and without this by-product)
    float q0 = 0.f, q1 = 0.f;
#pragma unroll
    for (int j = 0; j < A_F4; j++) {
      asm volatile("v_fmac_f32 %0, %2, %2\n v_fmac_f32 %1, %3, %3\n v_fmac_f32 %0, %4, %4\n v_fmac_f32 %1, %5, %5"
                   : "+v"(q0), "+v"(q1)
                   : "v"(ra[j].x), "v"(ra[j].y), "v"(ra[j].z), "v"(ra[j].w));
    }
    ssq += cf_tile * cf_tile * (q0 + q1);
  };
  // Per-segment, per-thread source pointers for the fast path (full K-step inside the segment, float4 loads):
  // rows/columns that are out of range read 16 zero bytes instead of branching.
  const float *aptr[A_F4], *bptr[B_F4];
  int astep[A_F4], bstep[B_F4];
  int ptr_seg = -1;
  auto setup_ptrs = [&]() {
    const GemmSeg sg = p.seg[sgi];
    const float *zero = reinterpret_cast<const float *>(&g_zero4);
#pragma unroll
    for (int j = 0; j < A_F4; j++) {
      const int idx = t + 256 * j, row = idx / KF4, m = m0 + row;
      const bool rv = (BM * BK / 4 % 256 == 0 || idx < BM * BK / 4) && m < p.M && m >= sg.m_lo && m < sg.m_hi;
      aptr[j] = rv ? p.A + sg.a_off + (long long)m * p.lda + (idx % KF4) * 4 : zero;
      astep[j] = rv ? 1 : 0;
    }
#pragma unroll
    for (int j = 0; j < B_F4; j++) {
      const int idx = t + 256 * j;
      bool rv;
      if (B_KC) {
        const int n = n0 + idx / KF4;
        rv = (BN * BK / 4 % 256 == 0 || idx < BN * BK / 4) && n < p.N;
        bptr[j] = rv ? p.B + sg.b_off + (long long)n * p.ldb + (idx % KF4) * 4 : zero;
        bstep[j] = rv ? 1 : 0;
      } else {
        const int kr = idx / (BN / 4), n = n0 + (idx % (BN / 4)) * 4;
        rv = (BN * BK / 4 % 256 == 0 || idx < BN * BK / 4) && n + 3 < p.N;
        bptr[j] = rv ? p.B + sg.b_off + (long long)kr * p.ldb + n : zero;
        bstep[j] = rv ? (int)p.ldb : 0;
      }
    }
    ptr_seg = seg;
  };
  // !B_KC: a ragged last column group (n + 3 >= N) needs the general path for the whole launch
  const bool fast_ok = VEC == 4 && (B_KC || p.N % 4 == 0);
  auto load_tile = [&]() {  // global -> registers for chunk (seg, kc)
    if (fast_ok && kc + BK <= klen) {
      if (ptr_seg != seg) setup_ptrs();
#pragma unroll
      for (int j = 0; j < A_F4; j++) ra[j] = *reinterpret_cast<const float4 *>(aptr[j] + (long long)kc * astep[j]);
#pragma unroll
      for (int j = 0; j < B_F4; j++) rb[j] = *reinterpret_cast<const float4 *>(bptr[j] + (long long)kc * bstep[j]);
      cf_tile = cf;
      return;
    }
    const GemmSeg sg = p.seg[sgi];
    const float *Ab = p.A + sg.a_off;
    const float *Bb = p.B + sg.b_off;
#pragma unroll
    for (int j = 0; j < A_F4; j++) {
      const int idx = t + 256 * j;
      const int row = idx / KF4, k = kc + (idx % KF4) * 4;
      const int m = m0 + row;
      const bool rv = (BM * BK / 4 % 256 == 0 || idx < BM * BK / 4) && m < p.M && m >= sg.m_lo && m < sg.m_hi;
      const float *ptr = Ab + (long long)m * p.lda + k;
      ra[j] = ld4(ptr, rv && k < klen, rv && k + 1 < klen, rv && k + 2 < klen, rv && k + 3 < klen, VEC == 4);
    }
    if (B_KC) {
#pragma unroll
      for (int j = 0; j < B_F4; j++) {
        const int idx = t + 256 * j;
        const int row = idx / KF4, k = kc + (idx % KF4) * 4;
        const int n = n0 + row;
        const bool rv = (BN * BK / 4 % 256 == 0 || idx < BN * BK / 4) && n < p.N;
        const float *ptr = Bb + (long long)n * p.ldb + k;
        rb[j] = ld4(ptr, rv && k < klen, rv && k + 1 < klen, rv && k + 2 < klen, rv && k + 3 < klen, VEC == 4);
      }
    } else {
      constexpr int NF4 = BN / 4;
#pragma unroll
      for (int j = 0; j < B_F4; j++) {
        const int idx = t + 256 * j;
        const int kr = idx / NF4, n = n0 + (idx % NF4) * 4;
        const bool rv = (BN * BK / 4 % 256 == 0 || idx < BN * BK / 4) && kc + kr < klen;
        const float *ptr = Bb + (long long)(kc + kr) * p.ldb + n;
        rb[j] = ld4(ptr, rv && n < p.N, rv && n + 1 < p.N, rv && n + 2 < p.N, rv && n + 3 < p.N, VEC == 4);
      }
    }
    cf_tile = cf;
  };
  auto store_tile = [&](int buf) {  // registers -> LDS
    float *as = As + buf * A_TILE, *bs = Bs + buf * B_TILE;
    if (p.sumsq) add_ssq();
    if (p.coef) {
#pragma unroll
      for (int j = 0; j < B_F4; j++) {
        rb[j].x *= cf_tile; rb[j].y *= cf_tile; rb[j].z *= cf_tile; rb[j].w *= cf_tile;
      }
    }
#pragma unroll
    for (int j = 0; j < A_F4; j++) {
      const int idx = t + 256 * j;
      if (BM * BK / 4 % 256 == 0 || idx < BM * BK / 4)
        *reinterpret_cast<float4 *>(as + (idx / KF4) * LDAS + (idx % KF4) * 4) = ra[j];
    }
#pragma unroll
    for (int j = 0; j < B_F4; j++) {
      const int idx = t + 256 * j;
      if (BN * BK / 4 % 256 == 0 || idx < BN * BK / 4) {
        if (B_KC)
          *reinterpret_cast<float4 *>(bs + (idx / KF4) * LDBS + (idx % KF4) * 4) = rb[j];
        else
          *reinterpret_cast<float4 *>(bs + (idx / (BN / 4)) * LDBS + (idx % (BN / 4)) * 4) = rb[j];
      }
    }
  };
  auto compute = [&](int buf) {
    const float *as = As + buf * A_TILE + (wm * TM * 32 + li) * LDAS + lh * 4;
    const float *bs = B_KC ? Bs + buf * B_TILE + (wn * TN * 32 + li) * LDBS + lh * 4
                           : Bs + buf * B_TILE + (lh * 4) * LDBS + wn * TN * 32 + li;
#pragma unroll
    for (int kg = 0; kg < BK / 8; kg++) {
      float4 a[TM], b[TN];
#pragma unroll
      for (int i = 0; i < TM; i++) a[i] = *reinterpret_cast<const float4 *>(as + i * 32 * LDAS + kg * 8);
#pragma unroll
      for (int i = 0; i < TN; i++) {
        if (B_KC) {
          b[i] = *reinterpret_cast<const float4 *>(bs + i * 32 * LDBS + kg * 8);
        } else {
          const float *q = bs + (kg * 8) * LDBS + i * 32;
          b[i] = make_float4(q[0], q[LDBS], q[2 * LDBS], q[3 * LDBS]);
        }
      }
#pragma unroll
      for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].x, b[j].x, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].y, b[j].y, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].z, b[j].z, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].w, b[j].w, acc[i][j], 0, 0, 0);
        }
    }
  };

  if (seg < p.nseg) {
    load_tile();
    store_tile(0);
    __syncthreads();
    int buf = 0;
    while (true) {
      kc += BK;
      if (kc >= klen) next_seg();
      const bool more = seg < p.nseg;
      if (more) load_tile();  // in flight while the MFMAs run
      compute(buf);
      if (!more) break;
      store_tile(buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }
  }

  // ---- epilogue.  C/D map of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5).
  // The accumulators go through LDS (reusing the staging buffers) so that C is read/written as whole
  // 16-byte-per-lane row segments instead of 64 four-byte accesses per lane.
  constexpr int LDCS = BN + 4;
  constexpr int SMEM_FLOATS = 2 * (A_TILE + B_TILE);
  constexpr int HALF = (BM * LDCS <= SMEM_FLOATS) ? BM : ((BM / 2) * LDCS <= SMEM_FLOATS ? BM / 2 : BM / 4);
  static_assert(HALF * LDCS <= SMEM_FLOATS, "epilogue tile does not fit the staging LDS");
  static_assert(HALF % (TM * 32) == 0, "a wave's rows must not straddle epilogue passes");
  float *Cs = smem;
  const bool cvec = p.c_vec != 0;
  __syncthreads();
  if (p.sumsq) {  // block total through LDS (the staging buffers are free now)
    double v = ssq;
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    double *red = reinterpret_cast<double *>(smem);
    if (lane == 0) red[wave] = v;
    __syncthreads();
    if (t == 0) p.sumsq[p.ksplit > 1 ? bx : bid] = (red[0] + red[1]) + (red[2] + red[3]);  // (no K split: entry = row tile)
    if (bx == 0)  // entries no block owns (the array is sized for a split-K launch)
      for (int i = gx + t; i < p.sumsq_cap; i += 256) p.sumsq[i] = 0.0;
    __syncthreads();
  }
  constexpr bool kColStats = 256 % (BN / 4) == 0 && (HALF * (BN / 4)) % 256 == 0;  // a thread keeps one float4 column group
  const bool colstats = kColStats && p.colstats && p.ksplit <= 1;
  float cs[4] = {0.f, 0.f, 0.f, 0.f}, cq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int pass = 0; pass < BM / HALF; pass++) {
    if ((wm * TM * 32) / HALF == pass) {
#pragma unroll
      for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++)
#pragma unroll
          for (int r = 0; r < 16; r++) {
            const int row = (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh - pass * HALF;
            Cs[row * LDCS + (wn * TN + j) * 32 + li] = acc[i][j][r];
          }
    }
    // Interior tiles (the whole tile inside M x N, 16-byte accesses): the values this pass adds to the accumulators -- the old C of an
    // accumulating launch, the fused addend -- are requested for several row segments at a time (eight for the 128-wide tile) before anything waits for them, and the
    // stores are not waited for either.  (The general loop below asks for one segment, waits -- also for the previous segment's store,
    // which shares the counter --, stores, and so on: sixteen trips to memory in a row per tile, most of what a K = 320 tile spent
    // outside its MFMAs when it carried an addend.)
    constexpr int kSeg = HALF * (BN / 4) / 256;  // row segments per thread and pass
    constexpr int kGrp = kSeg % 8 == 0 ? 8 : (kSeg % 5 == 0 ? 5 : (kSeg % 4 == 0 ? 4 : (kSeg % 2 == 0 ? 2 : 1)));  // requested together
    constexpr bool kFastShape = (HALF * (BN / 4)) % 256 == 0;
    const bool fast_tile = kFastShape && cvec && p.ksplit <= 1 && !p.serial_epilogue && m0 + BM <= p.M && n0 + BN <= p.N;
    if (fast_tile) {
      __syncthreads();
#pragma unroll
      for (int g = 0; g < kSeg; g += kGrp) {
        // bias or old C; the fused addend.  Branch-free (a segment with nothing to add reads 16 zero bytes), so that the requests
        // of a group leave back to back.  (Requested before the accumulators go to LDS, the first group's trip to memory would run
        // under the transposition -- but the extra live registers take the BK 16 kernel from three resident blocks per CU to two.)
        float4 pre[kGrp], addv[kGrp];
        const float *zero = reinterpret_cast<const float *>(&g_zero4);
#pragma unroll
        for (int u = 0; u < kGrp; u++) {
          const int idx = t + 256 * (g + u), m = m0 + pass * HALF + idx / (BN / 4), n = n0 + (idx % (BN / 4)) * 4;
          const float *pp = p.init_mode == 0 ? p.C + (long long)m * p.ldc + n : (p.init_mode == 1 ? p.bias + n : zero);
          const float *pa = (p.add && m >= p.add_lo && m < p.add_hi) ? p.add + (long long)(m - p.add_lo) * p.ldadd + n : zero;
          pre[u] = *reinterpret_cast<const float4 *>(pp);
          addv[u] = *reinterpret_cast<const float4 *>(pa);
        }
#pragma unroll
        for (int u = 0; u < kGrp; u++) {
          const int idx = t + 256 * (g + u), row = idx / (BN / 4), c4 = (idx % (BN / 4)) * 4;
          const int m = m0 + pass * HALF + row, n = n0 + c4;
          float4 v = *reinterpret_cast<const float4 *>(Cs + row * LDCS + c4);
          if constexpr (POST) {
            post_store4(p, m, n, v, pre[u], addv[u]);
            continue;
          }
          v.x += pre[u].x + p.add_scale * addv[u].x;
          v.y += pre[u].y + p.add_scale * addv[u].y;
          v.z += pre[u].z + p.add_scale * addv[u].z;
          v.w += pre[u].w + p.add_scale * addv[u].w;
          if (p.relu) { v.x = floor_keep_nan(v.x, 0.f); v.y = floor_keep_nan(v.y, 0.f); v.z = floor_keep_nan(v.z, 0.f); v.w = floor_keep_nan(v.w, 0.f); }
          *reinterpret_cast<float4 *>(p.C + (long long)m * p.ldc + n) = v;
          if (kColStats && colstats) {  // (kColStats: the thread's column group is the same in every segment)
            cs[0] += v.x; cs[1] += v.y; cs[2] += v.z; cs[3] += v.w;
            cq[0] += v.x * v.x; cq[1] += v.y * v.y; cq[2] += v.z * v.z; cq[3] += v.w * v.w;
          }
        }
      }
      if (pass + 1 < BM / HALF) __syncthreads();
      continue;
    }
    __syncthreads();
    for (int idx = t; idx < HALF * (BN / 4); idx += 256) {
      const int row = idx / (BN / 4), c4 = (idx % (BN / 4)) * 4;
      const int m = m0 + pass * HALF + row, n = n0 + c4;
      if (m >= p.M || n >= p.N) continue;
      float4 v = *reinterpret_cast<const float4 *>(Cs + row * LDCS + c4);
      if (p.ksplit > 1) {  // raw partial tile; the reduce kernel applies the epilogue
        const int ldp = (p.N + 3) & ~3;
        *reinterpret_cast<float4 *>(p.partial + ((long long)sp * p.M + m) * ldp + n) = v;
        continue;
      }
      if constexpr (POST) {  // (init_mode 1 or 2: rows_gemm() refuses an accumulating launch with this stage)
        if (cvec && n + 3 < p.N) {
          const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
          const float4 b = p.init_mode == 1 ? *reinterpret_cast<const float4 *>(p.bias + n) : z;
          const float4 o = (p.add && m >= p.add_lo && m < p.add_hi) ? *reinterpret_cast<const float4 *>(p.add + (long long)(m - p.add_lo) * p.ldadd + n) : z;
          post_store4(p, m, n, v, b, o);
        } else {
          const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int e = 0; e < 4; e++)
            if (n + e < p.N) post_store1(p, m, n + e, vv[e]);
        }
        continue;
      }
      float *c = p.C + (long long)m * p.ldc + n;
      if (cvec && n + 3 < p.N) {
        if (p.init_mode == 1) {
          const float4 b = *reinterpret_cast<const float4 *>(p.bias + n);
          v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
        } else if (p.init_mode == 0) {
          const float4 o = *reinterpret_cast<const float4 *>(c);
          v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
        }
        if (p.add && m >= p.add_lo && m < p.add_hi) {
          const float4 o = *reinterpret_cast<const float4 *>(p.add + (long long)(m - p.add_lo) * p.ldadd + n);
          v.x += p.add_scale * o.x; v.y += p.add_scale * o.y; v.z += p.add_scale * o.z; v.w += p.add_scale * o.w;
        }
        if (p.relu) { v.x = floor_keep_nan(v.x, 0.f); v.y = floor_keep_nan(v.y, 0.f); v.z = floor_keep_nan(v.z, 0.f); v.w = floor_keep_nan(v.w, 0.f); }
        *reinterpret_cast<float4 *>(c) = v;
        if (colstats) {
          cs[0] += v.x; cs[1] += v.y; cs[2] += v.z; cs[3] += v.w;
          cq[0] += v.x * v.x; cq[1] += v.y * v.y; cq[2] += v.z * v.z; cq[3] += v.w * v.w;
        }
      } else {
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
          if (n + e < p.N) {
            float x = vv[e];
            if (p.init_mode == 1) x += p.bias[n + e];
            else if (p.init_mode == 0) x += c[e];
            if (p.add && m >= p.add_lo && m < p.add_hi) x += p.add_scale * p.add[(long long)(m - p.add_lo) * p.ldadd + n + e];
            if (p.relu) x = floor_keep_nan(x, 0.f);
            c[e] = x;
            if (colstats) { cs[e] += x; cq[e] += x * x; }
          }
        }
      }
    }
    if (pass + 1 < BM / HALF) __syncthreads();
  }
  if (kColStats && colstats) {
    // thread t owns columns 4 (t % (BN/4)) .. +3 of every row it stored: lanes 32 apart share them when BN = 128, then the
    // four waves; one partial row per row tile
    constexpr int G = BN / 4;
    __syncthreads();
    float *red = smem;  // [256 / G][BN][2]
#pragma unroll
    for (int e = 0; e < 4; e++) {
      red[((t / G) * BN + (t % G) * 4 + e) * 2] = cs[e];
      red[((t / G) * BN + (t % G) * 4 + e) * 2 + 1] = cq[e];
    }
    __syncthreads();
    if (t < BN && n0 + t < p.N) {
      float a0 = 0.f, a1 = 0.f;
#pragma unroll
      for (int g = 0; g < 256 / G; g++) {
        a0 += red[(g * BN + t) * 2];
        a1 += red[(g * BN + t) * 2 + 1];
      }
      p.colstats[(long long)tile_m * p.N + n0 + t] = a0;
      p.colstats[((long long)p.colstats_stride + tile_m) * p.N + n0 + t] = a1;
    }
  }
}

template <int WM, int WN, int TM, int TN, int BK, bool B_KC, int VEC, int TAG = 0>
__global__ __launch_bounds__(256) void rows_gemm_kernel(const RowsGemmArgs p, int ntm, int ntn) {
  rows_gemm_block<WM, WN, TM, TN, BK, B_KC, VEC>(p, ntm, ntn, (int)blockIdx.x, (int)gridDim.x);
}
// the same GEMM with the inference epilogue (RowsGemmArgs::col_scale ...): plain launches, k-contiguous B
template <int WM, int WN, int TM, int TN, int BK, int VEC>
__global__ __launch_bounds__(256) void rows_gemm_post_kernel(const RowsGemmArgs p, int ntm, int ntn) {
  rows_gemm_block<WM, WN, TM, TN, BK, true, VEC, true>(p, ntm, ntn, (int)blockIdx.x, (int)gridDim.x);
}
// Grouped launch: task i owns the blocks [first[i], first[i + 1]) and runs them exactly as a launch of its own would (one column tile,
// no K split: its arguments say so).  The natural-gradient input-side statistics of a whole net at the recipes' minibatch: 33 launches
// of 26 .. 78 blocks each as one.
struct RowsGemmTasks {
  const RowsGemmArgs *args;  // device, ntasks
  const int *first;          // device, ntasks + 1
  int ntasks;
};
template <int WM, int WN, int TM, int TN, int BK, bool B_KC, int VEC>
__global__ __launch_bounds__(256) void rows_gemm_group_kernel(RowsGemmTasks g) {
  int lo = 0, hi = g.ntasks;  // the task whose block range holds blockIdx.x
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((int)blockIdx.x >= g.first[mid]) lo = mid;
    else hi = mid;
  }
  const int b0 = g.first[lo], nb = g.first[lo + 1] - b0;
  rows_gemm_block<WM, WN, TM, TN, BK, B_KC, VEC>(g.args[lo], nb, 1, (int)blockIdx.x - b0, nb);
}

// ------------------------------------------------------------------------ rows_gemm, split-bf16 arithmetic
// The same GEMM (arguments, K-segment iterator, epilogue) computed as a = a_hi + a_lo, b = b_hi + b_lo in bf16 with
//   a b ~ a_hi b_hi + a_hi b_lo + a_lo b_hi            (three v_mfma_f32_32x32x16_bf16 per 16 k, f32 accumulate):
// 16 mantissa bits per operand, products accurate to ~2^-16 relative, at 3/16 of the f32 MFMA's cycles per flop.
// The f32 operands are split when the staged tile goes to LDS (two bf16 planes per operand, 80-byte rows: conflict-free
// 16-byte fragment reads); lane (r, h) of a fragment holds k = 8h..8h+7 of row r (MI355X guide, bf16 operand maps).
// B must be k-contiguous (B_KC) and everything 16-byte aligned; rows_gemm() falls back to the f32 kernel otherwise.
template <int WM, int WN, int TM, int TN, int BK, int NP, int D, int TAG = 0>
__global__ __launch_bounds__(256, 2) void rows_gemm_x3_kernel(const RowsGemmArgs p, int ntm, int ntn) {
  constexpr int VEC = 4;
  constexpr bool B_KC = true;
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  constexpr int LDH = BK + 8;                 // bf16 per LDS row (80 bytes at BK = 32)
  constexpr int A_TILE = NP * BM * LDH / 2;   // floats per A buffer (NP planes)
  constexpr int B_TILE = NP * BN * LDH / 2;
  constexpr int A_F4 = (BM * BK / 4 + 255) / 256;
  constexpr int B_F4 = (BN * BK / 4 + 255) / 256;
  constexpr int KF4 = BK / 4;  // float4 per k-row of a k-contiguous tile
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *As = smem;               // [2][A_TILE]
  float *Bs = smem + 2 * A_TILE;  // [2][B_TILE]

  // XCD-aware tile order: blocks b and b+8 share an XCD (round-robin dispatch), so give each
  // XCD a contiguous run of logical tile ids; within it tile_n varies fastest so the blocks
  // that re-read the same A rows (and the taps' neighbouring rows) hit the same L2.
  const int nblk = ntm * ntn;
  int bid = blockIdx.x;
  {
    const int q = nblk / 8, r = nblk % 8, xcd = bid % 8, j = bid / 8;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
  }
  int sp = 0;
  if (p.ksplit > 1) {  // split-K launch: consecutive block ids share a tile
    sp = blockIdx.x % p.ksplit;
    bid = blockIdx.x / p.ksplit;
  }
  const long long k_begin = (long long)sp * p.kchunk, k_end = p.ksplit > 1 ? k_begin + p.kchunk : (1LL << 60);
  const int tile_m = bid / ntn, tile_n = bid % ntn;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int li = lane & 31, lh = lane >> 5;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; a++)
#pragma unroll
    for (int b = 0; b < TN; b++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[a][b][r] = 0.f;

  // ---- K iterator over (segment, chunk), skipping zero-coefficient segments
  // (a split-K block only visits the part of each segment inside its [k_begin, k_end) slice)
  int seg = -1, kc = 0, klen = 0;
  long long seg_kstart = 0, seg_knext = 0;
  float cf = 1.f;
  auto next_seg = [&]() {
    for (++seg; seg < p.nseg; ++seg) {
      seg_kstart = seg_knext;
      seg_knext += p.seg[seg].klen;
      cf = p.coef ? p.coef[seg] : 1.f;
      const long long lo = k_begin > seg_kstart ? k_begin - seg_kstart : 0;
      const long long hi = k_end < seg_knext ? k_end - seg_kstart : p.seg[seg].klen;
      if (cf != 0.f && hi > lo) {
        kc = (int)lo;
        klen = (int)hi;
        return;
      }
    }
    kc = 0;
    klen = 0;
  };
  next_seg();

  // D staged K-steps in registers: one being split into LDS, D - 1 in flight behind it.  A bf16 K-step is 4..5x shorter
  // than the f32 kernel's, far shorter than a global load's latency, so one step of prefetch leaves the MFMAs waiting.
  float4 ra[D][A_F4], rb[D][B_F4];
  // The tap coefficient (and the sum of squares of p.sumsq) is applied when a staged tile goes to LDS, not when it is
  // loaded: anything that touches ra/rb right after the loads would wait for them in front of the MFMAs they are
  // supposed to overlap with.
  float cf_tile[D];     // coefficient of the segment the tile in ra/rb[slot] was loaded from
  float ssq = 0.f;      // p.sumsq: running sum of (coef * a)^2 over everything this thread stages
  auto add_ssq = [&](const float4 (&xa)[A_F4], float c) {
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < A_F4; j++) q += xa[j].x * xa[j].x + xa[j].y * xa[j].y + xa[j].z * xa[j].z + xa[j].w * xa[j].w;
    ssq += c * c * q;
  };
  // Per-segment, per-thread source pointers for the fast path (full K-step inside the segment, float4 loads):
  // rows/columns that are out of range read 16 zero bytes instead of branching.
  const float *aptr[A_F4], *bptr[B_F4];
  int astep[A_F4], bstep[B_F4];
  int ptr_seg = -1;
  auto setup_ptrs = [&]() {
    const GemmSeg sg = p.seg[seg];
    const float *zero = reinterpret_cast<const float *>(&g_zero4);
#pragma unroll
    for (int j = 0; j < A_F4; j++) {
      const int idx = t + 256 * j, row = idx / KF4, m = m0 + row;
      const bool rv = (BM * BK / 4 % 256 == 0 || idx < BM * BK / 4) && m < p.M && m >= sg.m_lo && m < sg.m_hi;
      aptr[j] = rv ? p.A + sg.a_off + (long long)m * p.lda + (idx % KF4) * 4 : zero;
      astep[j] = rv ? 1 : 0;
    }
#pragma unroll
    for (int j = 0; j < B_F4; j++) {
      const int idx = t + 256 * j;
      bool rv;
      if (B_KC) {
        const int n = n0 + idx / KF4;
        rv = (BN * BK / 4 % 256 == 0 || idx < BN * BK / 4) && n < p.N;
        bptr[j] = rv ? p.B + sg.b_off + (long long)n * p.ldb + (idx % KF4) * 4 : zero;
        bstep[j] = rv ? 1 : 0;
      } else {
        const int kr = idx / (BN / 4), n = n0 + (idx % (BN / 4)) * 4;
        rv = (BN * BK / 4 % 256 == 0 || idx < BN * BK / 4) && n + 3 < p.N;
        bptr[j] = rv ? p.B + sg.b_off + (long long)kr * p.ldb + n : zero;
        bstep[j] = rv ? (int)p.ldb : 0;
      }
    }
    ptr_seg = seg;
  };
  // !B_KC: a ragged last column group (n + 3 >= N) needs the general path for the whole launch
  const bool fast_ok = VEC == 4 && (B_KC || p.N % 4 == 0);
  auto load_tile = [&](float4 (&ra)[A_F4], float4 (&rb)[B_F4], float &cf_tile) {  // global -> registers for chunk (seg, kc)
    if (fast_ok && kc + BK <= klen) {
      if (ptr_seg != seg) setup_ptrs();
#pragma unroll
      for (int j = 0; j < A_F4; j++) ra[j] = *reinterpret_cast<const float4 *>(aptr[j] + (long long)kc * astep[j]);
#pragma unroll
      for (int j = 0; j < B_F4; j++) rb[j] = *reinterpret_cast<const float4 *>(bptr[j] + (long long)kc * bstep[j]);
      cf_tile = cf;
      return;
    }
    const GemmSeg sg = p.seg[seg];
    const float *Ab = p.A + sg.a_off;
    const float *Bb = p.B + sg.b_off;
#pragma unroll
    for (int j = 0; j < A_F4; j++) {
      const int idx = t + 256 * j;
      const int row = idx / KF4, k = kc + (idx % KF4) * 4;
      const int m = m0 + row;
      const bool rv = (BM * BK / 4 % 256 == 0 || idx < BM * BK / 4) && m < p.M && m >= sg.m_lo && m < sg.m_hi;
      const float *ptr = Ab + (long long)m * p.lda + k;
      ra[j] = ld4(ptr, rv && k < klen, rv && k + 1 < klen, rv && k + 2 < klen, rv && k + 3 < klen, VEC == 4);
    }
    if (B_KC) {
#pragma unroll
      for (int j = 0; j < B_F4; j++) {
        const int idx = t + 256 * j;
        const int row = idx / KF4, k = kc + (idx % KF4) * 4;
        const int n = n0 + row;
        const bool rv = (BN * BK / 4 % 256 == 0 || idx < BN * BK / 4) && n < p.N;
        const float *ptr = Bb + (long long)n * p.ldb + k;
        rb[j] = ld4(ptr, rv && k < klen, rv && k + 1 < klen, rv && k + 2 < klen, rv && k + 3 < klen, VEC == 4);
      }
    } else {
      constexpr int NF4 = BN / 4;
#pragma unroll
      for (int j = 0; j < B_F4; j++) {
        const int idx = t + 256 * j;
        const int kr = idx / NF4, n = n0 + (idx % NF4) * 4;
        const bool rv = (BN * BK / 4 % 256 == 0 || idx < BN * BK / 4) && kc + kr < klen;
        const float *ptr = Bb + (long long)(kc + kr) * p.ldb + n;
        rb[j] = ld4(ptr, rv && n < p.N, rv && n + 1 < p.N, rv && n + 2 < p.N, rv && n + 3 < p.N, VEC == 4);
      }
    }
    cf_tile = cf;
  };
  auto store_tile = [&](float4 (&ra)[A_F4], float4 (&rb)[B_F4], const float cf_tile, int buf) {  // registers -> LDS
    float *as = As + buf * A_TILE, *bs = Bs + buf * B_TILE;
    if (p.sumsq) add_ssq(ra, cf_tile);
    if (p.coef) {
#pragma unroll
      for (int j = 0; j < B_F4; j++) {
        rb[j].x *= cf_tile; rb[j].y *= cf_tile; rb[j].z *= cf_tile; rb[j].w *= cf_tile;
      }
    }
    __bf16 *ah = reinterpret_cast<__bf16 *>(as), *bh = reinterpret_cast<__bf16 *>(bs);
#pragma unroll
    for (int j = 0; j < A_F4; j++) {
      const int idx = t + 256 * j;
      if (BM * BK / 4 % 256 == 0 || idx < BM * BK / 4) {
        bf16x4 pl[NP];
        split_bf16<NP>(ra[j], pl);
        const int o = (idx / KF4) * LDH + (idx % KF4) * 4;
#pragma unroll
        for (int q = 0; q < NP; q++) *reinterpret_cast<bf16x4 *>(ah + q * BM * LDH + o) = pl[q];
      }
    }
#pragma unroll
    for (int j = 0; j < B_F4; j++) {
      const int idx = t + 256 * j;
      if (BN * BK / 4 % 256 == 0 || idx < BN * BK / 4) {
        bf16x4 pl[NP];
        split_bf16<NP>(rb[j], pl);
        const int o = (idx / KF4) * LDH + (idx % KF4) * 4;
#pragma unroll
        for (int q = 0; q < NP; q++) *reinterpret_cast<bf16x4 *>(bh + q * BN * LDH + o) = pl[q];
      }
    }
  };
  auto compute = [&](int buf) {
    const __bf16 *ah = reinterpret_cast<const __bf16 *>(As + buf * A_TILE) + (wm * TM * 32 + li) * LDH + lh * 8;
    const __bf16 *bh = reinterpret_cast<const __bf16 *>(Bs + buf * B_TILE) + (wn * TN * 32 + li) * LDH + lh * 8;
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
          // every plane product a_q b_r with q + r < NP, smallest terms first and the leading term last
#pragma unroll
          for (int d = NP - 1; d >= 0; d--)
#pragma unroll
            for (int q = 0; q <= d; q++)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[q][i], b[d - q][j], acc[i][j], 0, 0, 0);
        }
    }
  };

  // One staged K-step beyond the one in LDS.  Measured on MI355X: a deeper register ring (2-4 steps, counted vmcnt waits
  // in a straight-line steady state) costs 60+ registers -> one block per CU or scratch, and ran 10-20 % slower than this
  // loop with two blocks per CU covering each other's load latency.
  if (seg < p.nseg) {
    load_tile(ra[0], rb[0], cf_tile[0]);
    store_tile(ra[0], rb[0], cf_tile[0], 0);
    __syncthreads();
    int buf = 0;
    while (true) {
      kc += BK;
      if (kc >= klen) next_seg();
      const bool more = seg < p.nseg;
      if (more) load_tile(ra[0], rb[0], cf_tile[0]);  // in flight while the MFMAs run
      compute(buf);
      if (!more) break;
      store_tile(ra[0], rb[0], cf_tile[0], buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }
  }

  // ---- epilogue.  C/D map of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5).
  // The accumulators go through LDS (reusing the staging buffers) so that C is read/written as whole
  // 16-byte-per-lane row segments instead of 64 four-byte accesses per lane.
  constexpr int LDCS = BN + 4;
  constexpr int SMEM_FLOATS = 2 * (A_TILE + B_TILE);
  constexpr int HALF = (BM * LDCS <= SMEM_FLOATS) ? BM : ((BM / 2) * LDCS <= SMEM_FLOATS ? BM / 2 : BM / 4);
  static_assert(HALF * LDCS <= SMEM_FLOATS, "epilogue tile does not fit the staging LDS");
  static_assert(HALF % (TM * 32) == 0, "a wave's rows must not straddle epilogue passes");
  float *Cs = smem;
  const bool cvec = p.c_vec != 0;
  __syncthreads();
  if (p.sumsq) {  // block total through LDS (the staging buffers are free now)
    double v = ssq;
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    double *red = reinterpret_cast<double *>(smem);
    if (lane == 0) red[wave] = v;
    __syncthreads();
    if (t == 0) p.sumsq[p.ksplit > 1 ? (int)blockIdx.x : bid] = (red[0] + red[1]) + (red[2] + red[3]);  // (no K split: entry = row tile)
    if (blockIdx.x == 0)  // entries no block owns (the array is sized for a split-K launch)
      for (int i = gridDim.x + t; i < p.sumsq_cap; i += 256) p.sumsq[i] = 0.0;
    __syncthreads();
  }
#pragma unroll
  for (int pass = 0; pass < BM / HALF; pass++) {
    if ((wm * TM * 32) / HALF == pass) {
#pragma unroll
      for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++)
#pragma unroll
          for (int r = 0; r < 16; r++) {
            const int row = (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh - pass * HALF;
            Cs[row * LDCS + (wn * TN + j) * 32 + li] = acc[i][j][r];
          }
    }
    {  // interior tiles: as in rows_gemm_kernel, the old C / bias / addend of several row segments requested together
      constexpr int kSeg = HALF * (BN / 4) / 256;
      constexpr int kGrp = kSeg % 8 == 0 ? 8 : (kSeg % 5 == 0 ? 5 : (kSeg % 4 == 0 ? 4 : (kSeg % 2 == 0 ? 2 : 1)));
      constexpr bool kFastShape = (HALF * (BN / 4)) % 256 == 0;
      if (kFastShape && cvec && p.ksplit <= 1 && !p.serial_epilogue && m0 + BM <= p.M && n0 + BN <= p.N) {
        __syncthreads();
#pragma unroll
        for (int g = 0; g < kSeg; g += kGrp) {
          float4 pre[kGrp], addv[kGrp];
          const float *zero = reinterpret_cast<const float *>(&g_zero4);
#pragma unroll
          for (int u = 0; u < kGrp; u++) {
            const int idx = t + 256 * (g + u), m = m0 + pass * HALF + idx / (BN / 4), n = n0 + (idx % (BN / 4)) * 4;
            const float *pp = p.init_mode == 0 ? p.C + (long long)m * p.ldc + n : (p.init_mode == 1 ? p.bias + n : zero);
            const float *pa = (p.add && m >= p.add_lo && m < p.add_hi) ? p.add + (long long)(m - p.add_lo) * p.ldadd + n : zero;
            pre[u] = *reinterpret_cast<const float4 *>(pp);
            addv[u] = *reinterpret_cast<const float4 *>(pa);
          }
#pragma unroll
          for (int u = 0; u < kGrp; u++) {
            const int idx = t + 256 * (g + u), row = idx / (BN / 4), c4 = (idx % (BN / 4)) * 4;
            const int m = m0 + pass * HALF + row, n = n0 + c4;
            float4 v = *reinterpret_cast<const float4 *>(Cs + row * LDCS + c4);
            v.x += pre[u].x + p.add_scale * addv[u].x;
            v.y += pre[u].y + p.add_scale * addv[u].y;
            v.z += pre[u].z + p.add_scale * addv[u].z;
            v.w += pre[u].w + p.add_scale * addv[u].w;
            if (p.relu) { v.x = floor_keep_nan(v.x, 0.f); v.y = floor_keep_nan(v.y, 0.f); v.z = floor_keep_nan(v.z, 0.f); v.w = floor_keep_nan(v.w, 0.f); }
            *reinterpret_cast<float4 *>(p.C + (long long)m * p.ldc + n) = v;
          }
        }
        if (pass + 1 < BM / HALF) __syncthreads();
        continue;
      }
    }
    __syncthreads();
    for (int idx = t; idx < HALF * (BN / 4); idx += 256) {
      const int row = idx / (BN / 4), c4 = (idx % (BN / 4)) * 4;
      const int m = m0 + pass * HALF + row, n = n0 + c4;
      if (m >= p.M || n >= p.N) continue;
      float4 v = *reinterpret_cast<const float4 *>(Cs + row * LDCS + c4);
      if (p.ksplit > 1) {  // raw partial tile; the reduce kernel applies the epilogue
        const int ldp = (p.N + 3) & ~3;
        *reinterpret_cast<float4 *>(p.partial + ((long long)sp * p.M + m) * ldp + n) = v;
        continue;
      }
      float *c = p.C + (long long)m * p.ldc + n;
      if (cvec && n + 3 < p.N) {
        if (p.init_mode == 1) {
          const float4 b = *reinterpret_cast<const float4 *>(p.bias + n);
          v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
        } else if (p.init_mode == 0) {
          const float4 o = *reinterpret_cast<const float4 *>(c);
          v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
        }
        if (p.add && m >= p.add_lo && m < p.add_hi) {
          const float4 o = *reinterpret_cast<const float4 *>(p.add + (long long)(m - p.add_lo) * p.ldadd + n);
          v.x += p.add_scale * o.x; v.y += p.add_scale * o.y; v.z += p.add_scale * o.z; v.w += p.add_scale * o.w;
        }
        if (p.relu) { v.x = floor_keep_nan(v.x, 0.f); v.y = floor_keep_nan(v.y, 0.f); v.z = floor_keep_nan(v.z, 0.f); v.w = floor_keep_nan(v.w, 0.f); }
        *reinterpret_cast<float4 *>(c) = v;
      } else {
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
          if (n + e < p.N) {
            float x = vv[e];
            if (p.init_mode == 1) x += p.bias[n + e];
            else if (p.init_mode == 0) x += c[e];
            if (p.add && m >= p.add_lo && m < p.add_hi) x += p.add_scale * p.add[(long long)(m - p.add_lo) * p.ldadd + n + e];
            if (p.relu) x = floor_keep_nan(x, 0.f);
            c[e] = x;
          }
        }
      }
    }
    if (pass + 1 < BM / HALF) __syncthreads();
  }
}

// epilogue of a split-K tail: C[m][n] = f(sum_sp partial[sp][m][n]) with the same init/bias/addend/ReLU rules
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const RowsGemmArgs p) {
  const int ldp = (p.N + 3) & ~3;
  const long long total = (long long)p.M * p.N;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int m = (int)(e / p.N), n = (int)(e % p.N);
    float v = 0.f;
#pragma unroll 4
    for (int sp = 0; sp < p.ksplit; sp++) v += p.partial[((long long)sp * p.M + m) * ldp + n];  // (unrolled: four requests in flight)
    float *c = p.C + (long long)m * p.ldc + n;
    if (p.init_mode == 1) v += p.bias[n];
    else if (p.init_mode == 0) v += *c;
    if (p.add && m >= p.add_lo && m < p.add_hi) v += p.add_scale * p.add[(long long)(m - p.add_lo) * p.ldadd + n];
    if (p.relu) v = floor_keep_nan(v, 0.f);
    *c = v;
  }
}

}  // namespace
}  // namespace tdnnf
