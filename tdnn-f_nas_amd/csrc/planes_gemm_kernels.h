// planes_gemm_kernels.h -- the GEMM kernel of the pre-split plane products and the finish of its split-K form (host side: planes_gemm.hip).
//
// A K step of a (BM x BN) tile is np CONTIGUOUS chunks of BM x 32 bytes of A and np of BN x 32 bytes of B (the P16 layout of
// planes_split_kernels.h): the kernel moves them with LDS-DMA (global_load_lds_dwordx4: no registers, no conversion, no LDS write
// instructions) into a ring of three stages, two K steps ahead of the one being multiplied, with counted vmcnt waits and one raw barrier
// per step (MI355X guide, "Pipelining across barriers").  One block of 8 waves per CU.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"
#include "planes_dev.h"
#include "planes_gemm.h"

namespace tdnnf {
namespace {

// LDS ring depth.  Three for every tile: the 256-row tiles of two planes would have room for four (128 KB, still one block per CU), measured
// on the trainer's shapes and in the step: no difference (the K loop is not bound by the latency of its loads) -- and 96 KB leave room beside it.
constexpr int kPlanesStages = 3;

// What follows from a tile's shape, for the kernel and for its launch: block = WM x WN waves, a wave owns TM x TN accumulator tiles of 32 x 32.
template <int NP, int WM, int WN, int TM, int TN>
struct PlanesTile {
  static constexpr int NT = WM * WN * 64, BM = WM * TM * 32, BN = WN * TN * 32;
  static constexpr int A_BYTES = NP * BM * 32, B_BYTES = NP * BN * 32, STAGE = A_BYTES + B_BYTES;
  static constexpr int PIECES = STAGE / 16, PPT = (PIECES + NT - 1) / NT;  // 16-byte pieces per stage / per thread
  static constexpr int STAGE_PAD = PPT * NT * 16;  // every thread copies PPT pieces per stage (the surplus ones into the pad): one vmcnt count for all waves
  static constexpr int NS = kPlanesStages;
  static constexpr int LDS_BYTES = NS * STAGE_PAD;
};

// ------------------------------------------------------------------------------------------------------ the GEMM
// ATR: the A operand is given by ROW-MAJOR planes of the matrix whose COLUMNS are the tile rows (a product that reduces over the
// matrix's rows, i.e. a weight gradient, without planes of the transpose): a K step is 16 consecutive matrix rows, the tile's 256
// columns are 16 K-block chunks of 16 x 32-byte row records, staged as [chunk pair][row 0..15][chunk parity][32 bytes] and read
// with ds_read_b64_tr_b16 (gfx950's transposing LDS read: a 16-lane group fetches 4 rows x 16 columns and every lane receives one
// column), two reads per operand register pair; rows of a 32-lane half cover 256 contiguous bytes: conflict-free.
// POST: the inference epilogue (PlanesGemmArgs::col_scale / col_offset / row_map and the addend AFTER the ReLU); the other
// instantiations do not read those fields and compile to what they were without it.
template <int NP, int WM, int WN, int TM, int TN, bool ATR = false, bool POST = false>
__global__ __launch_bounds__(WM *WN * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void planes_gemm_kernel(const PlanesGemmArgs p, int ntm, int ntn) {
  typedef typename Plane<NP>::V8 V8;
  typedef PlanesTile<NP, WM, WN, TM, TN> Tile;
  constexpr int NT = Tile::NT, BM = Tile::BM, BN = Tile::BN, A_BYTES = Tile::A_BYTES, PIECES = Tile::PIECES, PPT = Tile::PPT, STAGE_PAD = Tile::STAGE_PAD, NS = Tile::NS;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  // XCD-aware tile order (workgroups are dealt to the eight XCDs round-robin): each XCD a contiguous run of tiles, column tiles
  // (and taps) fastest so that neighbours share the A chunk, K splits slowest
  const int ntaps = p.ntap > 1 ? p.ntap : 1, ncol = ntn * ntaps, nsplit = p.ksplit > 1 ? p.ksplit : 1;
  const int nblk = ntm * ncol * nsplit;
  int bid = blockIdx.x;
  {
    const int q = nblk / 8, r = nblk % 8, xcd = bid % 8, j = bid / 8;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
  }
  const int sp = bid / (ntm * ncol), tile_m = (bid / ncol) % ntm, tcol = bid % ncol, tap = tcol / ntn, tile_n = tcol % ntn;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave / WN, wn = wave % WN, li = lane & 31, lh = lane >> 5;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; a++)
#pragma unroll
    for (int b = 0; b < TN; b++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[a][b][r] = 0.f;

  // ---- the stages in K order: (segment, K block).  This block multiplies stages [g_begin, g_begin + total).
  if (ntaps > 1 && p.skip_coef && p.skip_coef[tap] == 0.f) return;  // a tap with a zero coefficient (uniform-sample mode): its slab is not read either
  int all = 0;
  for (int s = 0; s < p.nseg; s++)
    if (!(ntaps <= 1 && p.skip_coef && p.skip_coef[s] == 0.f)) all += p.seg[s].nkb;
  // (alt_seg_order, as rows_gemm_kernel: odd row tiles visit the two taps in reverse order, so that the row block two neighbouring tiles
  // share is fetched by both in the same phase of the launch)
  const bool rev_seg = p.alt_seg_order && (tile_m & 1);
  const int g_begin = nsplit > 1 ? sp * p.kb_per_split : 0;
  const int total = nsplit > 1 ? max(0, min(all - g_begin, p.kb_per_split)) : all;
  const int tap_akb = ntaps > 1 ? p.tap_a_kb[tap] : 0, tap_bkb = ntaps > 1 ? p.tap_b_kb[tap] : 0;
  // what this thread copies per stage: piece q = t + NT j of the stage image [A planes | B planes]
  // (a plane chunk is contiguous in global memory as well: BM / BN row records of 32 bytes)
  int lds_off[PPT];
  bool isA[PPT], live[PPT];
  long long rel[PPT];  // byte offset inside the (kb, plane 0) chunk group of its operand, relative to the segment's first row
#pragma unroll
  for (int j = 0; j < PPT; j++) {
    const int q = t + NT * j;
    live[j] = q < PIECES;
    lds_off[j] = q * 16;
    isA[j] = q < A_BYTES / 16 || !live[j];
    const int w = isA[j] ? q : q - A_BYTES / 16;            // piece inside the operand's part
    const int rowsb = isA[j] ? BM * 2 : BN * 2;            // pieces per plane chunk
    const int pl = w / rowsb, inner = w % rowsb;
    rel[j] = live[j] ? ((long long)pl * (isA[j] ? p.RA : p.RB)) * 32 + (long long)inner * 16 : 0;  // (surplus pieces re-read the tile's first 16 bytes)
    if (ATR && isA[j] && live[j]) {  // piece `inner` of the image [chunk pair][row][parity][half]: K-block chunk 2 cp + parity, row record q
      const int cp = inner >> 6, rem = inner & 63, q = rem >> 2, par = (rem >> 1) & 1, h16 = rem & 1;
      rel[j] = ((long long)pl * p.RA + (long long)(2 * cp + par) * NP * p.RA + q) * 32 + h16 * 16;
    }
  }
  // Requests: every piece keeps a running source pointer, advanced by its operand's K-block stride after each stage; the segment
  // table (kernel arguments) is only read when a segment ends.
  const char *srcp[PPT];
  long long kstride[PPT];
#pragma unroll
  for (int j = 0; j < PPT; j++) kstride[j] = (ATR && isA[j]) ? 512 : (isA[j] ? p.RA : p.RB) * (32 * NP);  // (ATR: a K step is 16 rows of 32 bytes)
  int ld_seg = -1, ld_left = 0, ld_skip = g_begin;
  auto next_request_segment = [&]() {
    for (;;) {
      ld_seg++;
      if (ld_seg >= p.nseg) return;
      const int si = rev_seg ? p.nseg - 1 - ld_seg : ld_seg;
      if (ntaps <= 1 && p.skip_coef && p.skip_coef[si] == 0.f) continue;
      const PlanesSeg sg = p.seg[si];
      if (ld_skip >= sg.nkb) {  // (a split that starts behind this segment)
        ld_skip -= sg.nkb;
        continue;
      }
      ld_left = sg.nkb - ld_skip;
      const char *ga = ATR ? reinterpret_cast<const char *>(p.A) + ((long long)(m0 >> 4) * NP * p.RA + sg.a_row + 16LL * (sg.a_kb0 + tap_akb + ld_skip)) * 32
                           : reinterpret_cast<const char *>(p.A) + ((long long)(sg.a_kb0 + tap_akb + ld_skip) * NP * p.RA + sg.a_row + m0) * 32;
      const char *gb = reinterpret_cast<const char *>(p.B) + ((long long)(sg.b_kb0 + tap_bkb + ld_skip) * NP * p.RB + sg.b_row + n0) * 32;
      ld_skip = 0;
#pragma unroll
      for (int j = 0; j < PPT; j++) srcp[j] = (isA[j] ? ga : gb) + rel[j];
      return;
    }
  };
  next_request_segment();
  auto request_piece = [&](int slot, int j) {
    // (as an instruction the compiler does not see: it books the builtin as a flat access pending on BOTH counters and, knowing nothing of the
    // counted vmcnt waits below, turns every later lgkmcnt wait into lgkmcnt(0) -- the LDS reads could not be counted past each other)
    const unsigned m0v = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) void *)(smem + slot * STAGE_PAD + lds_off[j]));
    asm volatile("s_mov_b32 m0, %1\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(srcp[j]), "s"(m0v) : "memory");  // (m0 is a reserved register nothing else in these kernels uses)
    srcp[j] += kstride[j];
  };
  auto request_done = [&]() {
    if (--ld_left == 0) next_request_segment();
  };
  auto request = [&](int slot) {
#pragma unroll
    for (int j = 0; j < PPT; j++) request_piece(slot, j);
    request_done();
  };

  // fragment addressing: lane (li, lh) of a 32 x 32 x 16 MFMA holds k = 8 lh .. 8 lh + 7 of row li; the halves of a row record are
  // swapped when bit 3 of its absolute row is set (the segment's first row decides)
  int cs_seg = -1, cs_left = 0, cs_skip = g_begin;
  int a_off[TM], b_off[TN];  // byte offsets of this lane's fragments inside plane 0 of a stage
  auto next_compute_segment = [&]() {
    for (;;) {
      cs_seg++;
      if (cs_seg >= p.nseg) return;
      const int si = rev_seg ? p.nseg - 1 - cs_seg : cs_seg;
      if (ntaps <= 1 && p.skip_coef && p.skip_coef[si] == 0.f) continue;
      const PlanesSeg sg = p.seg[si];
      if (cs_skip >= sg.nkb) {
        cs_skip -= sg.nkb;
        continue;
      }
      cs_left = sg.nkb - cs_skip;
      cs_skip = 0;
      const int arow0 = (int)((sg.a_row + m0) & 15), brow0 = (int)((sg.b_row + n0) & 15);
#pragma unroll
      for (int i = 0; i < TM; i++) {
        const int row = wm * TM * 32 + i * 32 + li;
        a_off[i] = row * 32 + ((lh ^ (((row + arow0) >> 3) & 1)) << 4);
        if (ATR) {  // lane = 16 G + 4 q + pp: group G reads chunk parity G & 1, rows 8 (G >> 1) + q (then + 4), columns 4 pp ..
          const int G = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3, kg = G >> 1;
          a_off[i] = (wm * TM + i) * 1024 + (8 * kg + q) * 64 + (G & 1) * 32 + ((((pp >> 1) ^ kg) & 1) << 4) + ((pp & 1) << 3);
        }
      }
#pragma unroll
      for (int j = 0; j < TN; j++) {
        const int row = wn * TN * 32 + j * 32 + li;
        b_off[j] = A_BYTES + row * 32 + ((lh ^ (((row + brow0) >> 3) & 1)) << 4);
      }
      return;
    }
  };
  next_compute_segment();
  // One set of fragment registers.  (A second set, read for stage g + 1 while stage g is multiplied, was built and measured: no gain, spills
  // on the wide tiles.)
  auto read_a = [&](const char *st, int q, V8 (&a)[NP][TM]) {
#pragma unroll
    for (int i = 0; i < TM; i++) {
      if constexpr (ATR) {
        typedef __attribute__((address_space(3))) s16x4 *lds4;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(st + q * BM * 32 + a_off[i]));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(st + q * BM * 32 + a_off[i] + 256));
        union { s16x4 h[2]; V8 v; } u;
        u.h[0] = lo;
        u.h[1] = hi;
        a[q][i] = u.v;
      } else {
        a[q][i] = *reinterpret_cast<const V8 *>(st + q * BM * 32 + a_off[i]);
      }
    }
  };
  auto read_b = [&](const char *st, int q, V8 (&b)[NP][TN]) {
#pragma unroll
    for (int j = 0; j < TN; j++) b[q][j] = *reinterpret_cast<const V8 *>(st + q * BN * 32 + b_off[j]);
  };
  auto read_frags = [&](int slot, V8 (&a)[NP][TM], V8 (&b)[NP][TN]) {
    const char *st = smem + slot * STAGE_PAD;
#pragma unroll
    for (int q = 0; q < NP; q++) {
      read_b(st, q, b);
      read_a(st, q, a);
    }
    if (--cs_left == 0) next_compute_segment();  // (the NEXT read belongs to the next segment: its rows may swap other halves)
  };
  auto product = [&](const V8 (&a)[NP][TM], int qa, const V8 (&b)[NP][TN], int qb) {
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
      for (int j = 0; j < TN; j++) acc[i][j] = Plane<NP>::mfma(a[qa][i], b[qb][j], acc[i][j]);
  };
  auto multiply = [&](const V8 (&a)[NP][TM], const V8 (&b)[NP][TN]) {
    // the products a_q b_(d - q), d = np - 1 .. 0: smallest terms first, the leading term last
#pragma unroll
    for (int d = NP - 1; d >= 0; d--)
#pragma unroll
      for (int q = 0; q <= d; q++) product(a, q, b, d - q);
  };
  // the same product with the request pieces [jlo, jhi) of `slot` issued between its MFMAs, evenly spaced (a piece issued alone costs the
  // wave ~60 cycles, several in a row behind a barrier 100-185 each -- with both waves of a SIMD there together the matrix pipe idles)
  auto product_req = [&](const V8 (&a)[NP][TM], int qa, const V8 (&b)[NP][TN], int qb, bool req, int slot, int jlo, int jhi) {
    constexpr int total_m = TM * TN;
    const int np = jhi - jlo;
#pragma unroll
    for (int k = 0; k < total_m; k++) {
      acc[k / TN][k % TN] = Plane<NP>::mfma(a[qa][k / TN], b[qb][k % TN], acc[k / TN][k % TN]);
#pragma unroll
      for (int n = 0; n < PPT; n++)
        if (n < np && k == ((n + 1) * total_m) / (np + 1) - 1) {
          __builtin_amdgcn_sched_barrier(0);
          if (req) request_piece(slot, jlo + n);
          __builtin_amdgcn_sched_barrier(0);
        }
    }
  };
  // wait until at most `k` stages' requests of this thread are outstanding (k <= NS - 1; uniform)
  auto wait_stages = [&](int k) {
    static_assert(NS == 3 && (NS - 1) * PPT <= 63, "vmcnt is a 6-bit count; the arms below are those of a ring of three");
    if (k == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PPT) : "memory");
    else if (k == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PPT) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  };

  if constexpr (NP == 2) {
    // Two planes, one register set, no exposed LDS phase: a K step's three products are ordered l h', h h', h l' and the fragments of the NEXT
    // stage are read into each operand's registers as soon as its last product of THIS stage has been issued -- l after the first product,
    // h' after the second, h and l' after the third -- so every LDS read has eight MFMAs (256 cycles of the matrix pipe) or more between
    // its issue and its first use.  (Read all at once behind the barrier, the twelve reads of a step sat in front of its MFMAs in both
    // waves of a SIMD together: the compute phase alone ran at 1.26 us per K step of a 256 x 256 tile where the MFMAs take 0.65-0.8.)
    // The barrier sits behind the first product: stage g + 1 has landed for everybody and everybody's reads of stage g are complete
    // (lgkmcnt(0): they were issued a product earlier), so slot g % NS takes stage g + NS.
    V8 fa[NP][TM], fb[NP][TN];
#pragma unroll
    for (int i = 0; i < NS; i++)
      if (total > i) request(i);
    if (total > 0) {
      wait_stages(min(NS - 1, total - 1));
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0), as an instruction the compiler's counter model sees: kernel-argument loads still pending here
                                           // (scalar loads share the counter and return out of order) would make it wait for ALL LDS reads at the loop head
      read_a(smem, 1, fa);  // (in the loop's order: the first product's operands are the oldest reads on either way into the loop)
      read_b(smem, 0, fb);
      __builtin_amdgcn_sched_barrier(0);
      read_a(smem, 0, fa);
      read_b(smem, 1, fb);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (total > 0) {
      product(fa, 1, fb, 0);
      __builtin_amdgcn_sched_barrier(0);
      // (the loop begins behind step g's first product, at its barrier: the one place of a step where no LDS read is outstanding, so the
      // compiler's wait-count model, which gives up precision across a loop's back edge, has nothing to be conservative about)
      for (int g = 0; g + 1 < total; g++) {
        const char *st = smem + ((g + 1) % NS) * STAGE_PAD;
        wait_stages(min(NS - 2, total - g - 2));
        __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
        __builtin_amdgcn_s_barrier();
        if (--cs_left == 0) next_compute_segment();  // the fragment offsets of stage g + 1 (the segment table is read with scalar loads, which share the LDS reads' counter)
        const bool req = g + NS < total;
        read_a(st, 1, fa);
        __builtin_amdgcn_sched_barrier(0);
        product_req(fa, 0, fb, 0, req, g % NS, 0, PPT / 2);
        __builtin_amdgcn_sched_barrier(0);
        read_b(st, 0, fb);
        __builtin_amdgcn_sched_barrier(0);
        product_req(fa, 0, fb, 1, req, g % NS, PPT / 2, PPT);
        if (req) request_done();
        __builtin_amdgcn_sched_barrier(0);
        read_a(st, 0, fa);
        read_b(st, 1, fb);
        __builtin_amdgcn_sched_barrier(0);
        product(fa, 1, fb, 0);  // (of step g + 1)
        __builtin_amdgcn_sched_barrier(0);
      }
      product(fa, 0, fb, 0);
      product(fa, 0, fb, 1);
    }
  } else {
    // One register set (tiles whose accumulators leave no room for a second): stage g is read and multiplied behind the barrier
    // that follows its wait; NS - 1 stages are in flight meanwhile.
    V8 fa[NP][TM], fb[NP][TN];
#pragma unroll
    for (int i = 0; i < NS - 1; i++)
      if (total > i) request(i);
    for (int g = 0; g < total; g++) {
      wait_stages(min(NS - 2, total - g - 1));
      __builtin_amdgcn_s_barrier();  // everybody's pieces of stage g are in LDS; everybody is done reading stage g - 1
      if (g + NS - 1 < total) request((g + NS - 1) % NS);  // into the slot stage g - 1 used
      read_frags(g % NS, fa, fb);
      multiply(fa, fb);
    }
  }

  // ---- epilogue: straight from the accumulators (C/D map: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)):
  // a store instruction writes two 128-byte row segments
  if (nsplit > 1) {  // raw partial tile into this split's slab (the caller reduces, scales, accumulates)
    float *P = p.partial + (long long)sp * p.partial_stride + (long long)tap * p.tap_off_p;
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
      for (int j = 0; j < TN; j++) {
        const int n = n0 + (wn * TN + j) * 32 + li;
        if (n >= p.N) continue;
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int m = m0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          if (m < p.M) P[(long long)m * p.ldp_m + (long long)n * p.ldp_n] = acc[i][j][r];
        }
      }
    return;
  }
  float sc = 1.0f;
  if (NP == 2) sc = (p.scale_a ? p.scale_a[1] : 1.0f) * (p.scale_b ? p.scale_b[1] : 1.0f);
  // Row-contiguous epilogue: a wave passes its 32 x 64 accumulator chunks through a private LDS slab ([32][64 + 4] floats, in the ring's
  // memory) and works on them as rows -- 16 lanes x 16 bytes per row, four rows per instruction -- so that the output, the `+=` operand and
  // the bypass addend move as 256-byte row segments in dwordx4 accesses, the loads of a chunk's eight row groups issued together.  (Straight
  // from the accumulators a lane owns one column: 4-byte accesses, 128 of them per thread and operand, each behind its own bounds test --
  // the .linear backward-data GEMM, which adds the bypass derivative, took 675 us where the same product without an addend took 280.)
  // Chunks at the ragged right edge, and operands that are not 16-byte aligned, take the element-wise path.
  constexpr int CW = 64, LDW = CW + 4, NCH = (TN + 1) / 2;
  const bool vec_ok = (reinterpret_cast<uintptr_t>(p.C) & 15) == 0 && p.ldc % 4 == 0 && p.tap_off_c % 4 == 0 &&
                      (!p.add || ((reinterpret_cast<uintptr_t>(p.add) & 15) == 0 && p.ldadd % 4 == 0)) &&
                      (p.init_mode != 1 || (reinterpret_cast<uintptr_t>(p.bias) & 15) == 0);
  float cs1[TN], cs2[TN];      // column sums / sums of squares of what this lane stores, element-wise chunks (p.colstats)
  float vs1[NCH][4], vs2[NCH][4];  // the same, row-contiguous chunks: columns 4 (lane & 15) .. + 3 of the chunk
#pragma unroll
  for (int j = 0; j < TN; j++) cs1[j] = cs2[j] = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; c++)
#pragma unroll
    for (int e = 0; e < 4; e++) vs1[c][e] = vs2[c][e] = 0.f;
  __builtin_amdgcn_s_barrier();  // every wave has read its last fragments: the ring's memory is free
  float *scr = reinterpret_cast<float *>(smem) + wave * (32 * LDW);
  const int rr = lane >> 4, c4 = (lane & 15) * 4;
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int ch = 0; ch < NCH; ch++) {
      const int j0 = ch * 2, nj = (TN - j0) < 2 ? (TN - j0) : 2, ncol = nj * 32;
      const int nw = n0 + (wn * TN + j0) * 32;  // first column of the chunk
      if (nw >= p.N) continue;
      if (vec_ok && nw + ncol <= p.N) {
#pragma unroll
        for (int jj = 0; jj < nj; jj++)
#pragma unroll
          for (int r = 0; r < 16; r++) scr[((r & 3) + 8 * (r >> 2) + 4 * lh) * LDW + jj * 32 + li] = acc[i][j0 + jj][r];
        const bool col_on = c4 < ncol;
        const int n = nw + c4;
        float4 bias4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p.init_mode == 1 && col_on) bias4 = *reinterpret_cast<const float4 *>(p.bias + n);
        float csc[4] = {1.f, 1.f, 1.f, 1.f}, cof[4] = {0.f, 0.f, 0.f, 0.f};
        if constexpr (POST) {
          if (p.col_scale && col_on) {
#pragma unroll
            for (int e = 0; e < 4; e++) {
              csc[e] = p.col_scale[n + e];
              cof[e] = p.col_offset[n + e];
            }
          }
        }
        const int mrow0 = m0 + (wm * TM + i) * 32 + rr;
        float4 addv[8], cold[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
          const int m = mrow0 + 4 * q;
          addv[q] = make_float4(0.f, 0.f, 0.f, 0.f);
          cold[q] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (col_on && m < p.M) {
            if (p.add && m >= p.add_lo && m < p.add_hi) addv[q] = *reinterpret_cast<const float4 *>(p.add + (long long)(m - p.add_lo) * p.ldadd + n);
            if (p.init_mode == 0) cold[q] = *reinterpret_cast<const float4 *>(p.C + (long long)m * p.ldc + (long long)tap * p.tap_off_c + n);
          }
        }
#pragma unroll
        for (int q = 0; q < 8; q++) {
          const int m = mrow0 + 4 * q;
          if (!(col_on && m < p.M)) continue;
          const float4 a4 = *reinterpret_cast<const float4 *>(scr + (rr + 4 * q) * LDW + c4);
          float v[4] = {a4.x * sc + bias4.x + cold[q].x + p.add_scale * addv[q].x, a4.y * sc + bias4.y + cold[q].y + p.add_scale * addv[q].y,
                        a4.z * sc + bias4.z + cold[q].z + p.add_scale * addv[q].z, a4.w * sc + bias4.w + cold[q].w + p.add_scale * addv[q].w};
          if constexpr (POST) {
            const float b4[4] = {bias4.x, bias4.y, bias4.z, bias4.w}, s4[4] = {a4.x, a4.y, a4.z, a4.w}, d4[4] = {addv[q].x, addv[q].y, addv[q].z, addv[q].w};
            const int mo = p.row_map ? p.row_map[m] : m;
            if (mo < 0) continue;
#pragma unroll
            for (int e = 0; e < 4; e++) {
              float x = s4[e] * sc + b4[e];
              if (p.relu) x = floor_keep_nan(x, 0.f);
              if (p.col_scale) x = x * csc[e] + cof[e];
              if (p.add) x += p.add_scale * d4[e];
              v[e] = x;
              vs1[ch][e] += x;
              vs2[ch][e] += x * x;
            }
            *reinterpret_cast<float4 *>(p.C + (long long)mo * p.ldc + n) = make_float4(v[0], v[1], v[2], v[3]);
            continue;
          }
#pragma unroll
          for (int e = 0; e < 4; e++) {
            if (p.relu) v[e] = floor_keep_nan(v[e], 0.f);
            vs1[ch][e] += v[e];
            vs2[ch][e] += v[e] * v[e];
          }
          *reinterpret_cast<float4 *>(p.C + (long long)m * p.ldc + (long long)tap * p.tap_off_c + n) = make_float4(v[0], v[1], v[2], v[3]);
        }
      } else {
#pragma unroll
        for (int jj = 0; jj < nj; jj++) {
          const int j = j0 + jj;
          const int n = n0 + (wn * TN + j) * 32 + li;
          if (n >= p.N) continue;
          const float bias = p.init_mode == 1 ? p.bias[n] : 0.f;
#pragma unroll
          for (int r = 0; r < 16; r++) {
            const int m = m0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (m >= p.M) continue;
            if constexpr (POST) {
              const int mo = p.row_map ? p.row_map[m] : m;
              if (mo < 0) continue;
              float x = acc[i][j][r] * sc + bias;
              if (p.relu) x = floor_keep_nan(x, 0.f);
              if (p.col_scale) x = x * p.col_scale[n] + p.col_offset[n];
              if (p.add && m >= p.add_lo && m < p.add_hi) x += p.add_scale * p.add[(long long)(m - p.add_lo) * p.ldadd + n];
              p.C[(long long)mo * p.ldc + n] = x;
              cs1[j] += x;
              cs2[j] += x * x;
              continue;
            }
            float *c = p.C + (long long)m * p.ldc + (long long)tap * p.tap_off_c + n;
            float v = acc[i][j][r] * sc + bias;
            if (p.init_mode == 0) v += *c;
            if (p.add && m >= p.add_lo && m < p.add_hi) v += p.add_scale * p.add[(long long)(m - p.add_lo) * p.ldadd + n];
            if (p.relu) v = floor_keep_nan(v, 0.f);
            *c = v;
            cs1[j] += v;
            cs2[j] += v * v;
          }
        }
      }
    }
  if (p.colstats) {  // one partial row per row tile: the lanes that hold the same columns first, the WM wave rows through LDS (fixed order)
#pragma unroll
    for (int j = 0; j < TN; j++) {
      cs1[j] += __shfl_xor(cs1[j], 32, 64);
      cs2[j] += __shfl_xor(cs2[j], 32, 64);
    }
#pragma unroll
    for (int c = 0; c < NCH; c++)
#pragma unroll
      for (int e = 0; e < 4; e++) {
        vs1[c][e] += __shfl_xor(vs1[c][e], 16, 64);
        vs1[c][e] += __shfl_xor(vs1[c][e], 32, 64);
        vs2[c][e] += __shfl_xor(vs2[c][e], 16, 64);
        vs2[c][e] += __shfl_xor(vs2[c][e], 32, 64);
      }
    __syncthreads();  // (every wave is done with its slab)
    float *red = reinterpret_cast<float *>(smem);  // [wm][2][BN]
#pragma unroll
    for (int ch = 0; ch < NCH; ch++) {
      const int j0 = ch * 2, nj = (TN - j0) < 2 ? (TN - j0) : 2, ncol = nj * 32;
      const int nw = n0 + (wn * TN + j0) * 32;
      if (nw >= p.N) continue;
      if (vec_ok && nw + ncol <= p.N) {
        if (rr == 0 && c4 < ncol) {
#pragma unroll
          for (int e = 0; e < 4; e++) {
            red[(wm * 2 + 0) * BN + (wn * TN + j0) * 32 + c4 + e] = vs1[ch][e];
            red[(wm * 2 + 1) * BN + (wn * TN + j0) * 32 + c4 + e] = vs2[ch][e];
          }
        }
      } else if (lh == 0) {
#pragma unroll
        for (int jj = 0; jj < nj; jj++) {
          const int nl = (wn * TN + j0 + jj) * 32 + li;
          red[(wm * 2 + 0) * BN + nl] = cs1[j0 + jj];
          red[(wm * 2 + 1) * BN + nl] = cs2[j0 + jj];
        }
      }
    }
    __syncthreads();
    for (int nl = t; nl < BN; nl += NT) {
      const int n = n0 + nl;
      if (n >= p.N) continue;
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int w = 0; w < WM; w++) {
        s1 += red[(w * 2 + 0) * BN + nl];
        s2 += red[(w * 2 + 1) * BN + nl];
      }
      p.colstats[(long long)tile_m * p.N + n] = s1;
      p.colstats[(long long)(p.colstats_stride + tile_m) * p.N + n] = s2;
    }
  }
}

__global__ __launch_bounds__(256) void planes_splitk_finish_kernel(const PlanesGemmArgs p) {
  const long long total = (long long)p.M * p.N;
  float sc = 1.0f;
  if (p.np == 2) sc = (p.scale_a ? p.scale_a[1] : 1.0f) * (p.scale_b ? p.scale_b[1] : 1.0f);
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int m = (int)(e / p.N), n = (int)(e % p.N);
    float v = 0.f;
#pragma unroll 4
    for (int sp = 0; sp < p.ksplit; sp++) v += p.partial[(long long)sp * p.partial_stride + (long long)m * p.ldp_m + n];
    v *= sc;
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
