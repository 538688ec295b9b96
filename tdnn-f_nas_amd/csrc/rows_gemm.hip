// rows_gemm.hip -- host side of the rows GEMM (gemm_f32.h): tile choice, the launch planner that balances rounds of resident
// blocks with split-K launches, the router onto the pre-split plane kernels, the grouped launch.  Kernels: rows_gemm_kernels.h.
#include <algorithm>
#include <cstring>
#include <vector>

#include "colreduce.h"
#include "common.h"
#include "device.h"
#include "gemm_f32.h"
#include "gemm_ring.h"
#include "launch_forms.h"
#include "planes_gemm.h"
#include "rows_gemm_kernels.h"

namespace tdnnf {
namespace {

// what the scopes of gemm_f32.h install
float *g_scratch_override = nullptr;
size_t g_scratch_override_bytes = 0;
int g_gemm_prec = 0;
const float *g_tw_w = nullptr, *g_tw_wt = nullptr;
long long g_tw_n = 0;

// ---- what the planner asks of a call's K segments
struct KRange {
  long long ktot;  // the concatenated reduction length
  bool k4;         // every segment a multiple of 4 long (one segment: only the very end of K is ragged -- slow path of the last chunk)
};
KRange k_range(const RowsGemmArgs &a) {
  KRange k{0, true};
  for (int i = 0; i < a.nseg; i++) {
    k.ktot += a.seg[i].klen;
    k.k4 = k.k4 && (a.seg[i].klen % 4 == 0 || a.nseg == 1);
  }
  return k;
}
// two taps of one matrix: same reduction length, A offsets whole rows apart (alt_seg_order, rows_gemm_kernels.h)
bool is_two_tap_shift(const RowsGemmArgs &a) {
  return a.nseg == 2 && a.seg[0].klen == a.seg[1].klen && a.lda > 0 && a.seg[0].a_off != a.seg[1].a_off && (a.seg[1].a_off - a.seg[0].a_off) % a.lda == 0;
}
// output rows of [0, M) for which the segment's A is defined
int usable_rows(const GemmSeg &sg, int M) {
  const int lo = sg.m_lo > 0 ? sg.m_lo : 0, hi = sg.m_hi < M ? sg.m_hi : M;
  return hi > lo ? hi - lo : 0;
}
// the float4 path needs 16-byte aligned rows and segment starts; ragged tails fall back per float4
bool operands_vec4(const RowsGemmArgs &a) {
  bool vec = aligned16(a.A) && aligned16(a.B) && a.lda % 4 == 0 && a.ldb % 4 == 0;
  for (int i = 0; i < a.nseg; i++) vec = vec && a.seg[i].a_off % 4 == 0 && a.seg[i].b_off % 4 == 0;
  return vec;
}

// ---- dynamic LDS of a tile: double-buffered A and B tiles, rows padded by 4 floats (f32) / 8 bf16 (NP planes per operand)
template <int BM, int BN, int BK>
constexpr size_t rows_lds_bytes(bool b_kc) {
  return sizeof(float) * 2 * (BM * (BK + 4) + (b_kc ? BN * (BK + 4) : BK * (BN + 4)));
}
template <int BM, int BN, int BK, int NP>
constexpr size_t rows_x3_lds_bytes() {
  return sizeof(__bf16) * 2 * NP * (size_t)(BM + BN) * (BK + 8);
}

// ---- launch-form counters (launch_forms.h).  The launch sites below record what they launched: the arithmetic (0 exact f32, 1 bf16x3,
// 2 bf16x6) of the calling thread's last kernel, for the planner to count its form under, and vec4 / scalar loads per launch
thread_local int t_launched_arith = 0;
inline void note_launch(int arith, bool vec) {
  t_launched_arith = arith;
  count_form(vec ? kRowsVec4Launches : kRowsScalarLaunches);
}
template <int WM, int WN, int TM, int TN, int BK>
void count_rows_form(int form) {  // (after the launch: under the arithmetic that ran)
  count_form(rows_form_index(rows_tile_index<WM, WN, TM, TN, BK>(), t_launched_arith, form));
}

// ---- kernel launches.  TAG 1 (rows_gemm_kernels.h): the launches booked to the natural-gradient class
template <int WM, int WN, int TM, int TN, int BK, int NP, int TAG>
void launch_rows_x3_tagged(dim3 grid, const RowsGemmArgs &a, int ntm, int ntn, hipStream_t s) {
  constexpr int D = 1;  // staged K-steps beyond the one in LDS.  Measured: D = 2 needs > 256 registers (one block per CU, or
                        // scratch) and runs 20 % slower than D = 1 with two blocks per CU covering each other's load latency
  constexpr size_t lds = rows_x3_lds_bytes<WM * TM * 32, WN * TN * 32, BK, NP>();
  static const bool opted = opt_in_lds(rows_gemm_x3_kernel<WM, WN, TM, TN, BK, NP, D, TAG>, lds);
  (void)opted;
  note_launch(NP - 1, true);
  hipLaunchKernelGGL((rows_gemm_x3_kernel<WM, WN, TM, TN, BK, NP, D, TAG>), grid, dim3(256), lds, s, a, ntm, ntn);
}

template <int WM, int WN, int TM, int TN, int BK, int TAG>
void launch_rows_kernel_tagged(dim3 grid, const RowsGemmArgs &a, int ntm, int ntn, bool b_kc, bool vec, hipStream_t s) {
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  constexpr size_t lds_kc = rows_lds_bytes<BM, BN, BK>(true), lds_nc = rows_lds_bytes<BM, BN, BK>(false);
  static const bool opted = opt_in_lds(rows_gemm_kernel<WM, WN, TM, TN, BK, true, 4, TAG>, lds_kc) && opt_in_lds(rows_gemm_kernel<WM, WN, TM, TN, BK, true, 1, TAG>, lds_kc) &&
                            opt_in_lds(rows_gemm_kernel<WM, WN, TM, TN, BK, false, 4, TAG>, lds_nc) && opt_in_lds(rows_gemm_kernel<WM, WN, TM, TN, BK, false, 1, TAG>, lds_nc);
  (void)opted;
  const dim3 block(256);
  note_launch(0, vec);
  if (b_kc) {
    if (vec) hipLaunchKernelGGL((rows_gemm_kernel<WM, WN, TM, TN, BK, true, 4, TAG>), grid, block, lds_kc, s, a, ntm, ntn);
    else hipLaunchKernelGGL((rows_gemm_kernel<WM, WN, TM, TN, BK, true, 1, TAG>), grid, block, lds_kc, s, a, ntm, ntn);
  } else {
    if (vec) hipLaunchKernelGGL((rows_gemm_kernel<WM, WN, TM, TN, BK, false, 4, TAG>), grid, block, lds_nc, s, a, ntm, ntn);
    else hipLaunchKernelGGL((rows_gemm_kernel<WM, WN, TM, TN, BK, false, 1, TAG>), grid, block, lds_nc, s, a, ntm, ntn);
  }
}
// every rows_gemm_kernel launch goes through here
template <int WM, int WN, int TM, int TN, int BK>
void launch_rows_kernel(dim3 grid, const RowsGemmArgs &a, int ntm, int ntn, bool b_kc, bool vec, hipStream_t s) {
  const bool ng = prof_class_override() == 3;
  if (a.prec == 1 && b_kc && vec) {  // split-bf16 arithmetic, two planes (three products)
    if (ng) launch_rows_x3_tagged<WM, WN, TM, TN, BK, 2, 1>(grid, a, ntm, ntn, s);
    else launch_rows_x3_tagged<WM, WN, TM, TN, BK, 2, 0>(grid, a, ntm, ntn, s);
    return;
  }
  if (a.prec == 3 && b_kc && vec) {  // three planes (six products): f32-equivalent
    if constexpr (BK == 16) {
      if (ng) launch_rows_x3_tagged<WM, WN, TM, TN, BK, 3, 1>(grid, a, ntm, ntn, s);
      else launch_rows_x3_tagged<WM, WN, TM, TN, BK, 3, 0>(grid, a, ntm, ntn, s);
      return;
    }
  }
  if (ng) launch_rows_kernel_tagged<WM, WN, TM, TN, BK, 1>(grid, a, ntm, ntn, b_kc, vec, s);
  else launch_rows_kernel_tagged<WM, WN, TM, TN, BK, 0>(grid, a, ntm, ntn, b_kc, vec, s);
}

template <int WM, int WN, int TM, int TN>
constexpr bool kRingTile = (WM == 2 && WN == 2 && TM == 2 && TN == 2) || (WM == 4 && WN == 1 && TM == 1 && TN == 5);
inline bool ring_applies(const RowsGemmArgs &a, bool b_kc, bool vec, int tile_cols) {
  return prof_class_override() != 3 && (tile_cols == 128 || rows_gemm_ring_mode() >= 2) && rows_gemm_ring_ok(a, b_kc, vec);
}

// (form: what a launch of the tile kernel is counted as; the ring counts as itself)
template <int WM, int WN, int TM, int TN, int BK>
hipError_t launch_rows(const RowsGemmArgs &a, bool b_kc, bool vec, hipStream_t s, int form = kFormPlain) {
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  const int ntm = (a.M + BM - 1) / BM, ntn = (a.N + BN - 1) / BN;
  if constexpr (kRingTile<WM, WN, TM, TN>) {  // the persistent LDS-DMA-ring form (gemm_ring.hip) where it applies
    if (ring_applies(a, b_kc, vec, BN)) {
      note_launch(0, true);  // (the ring is exact f32 on 16-byte loads: rows_gemm_ring_ok)
      count_rows_form<WM, WN, TM, TN, BK>(kFormRing);
      return rows_gemm_ring(a, b_kc, BN, s);
    }
  }
  launch_rows_kernel<WM, WN, TM, TN, BK>(dim3(ntm * ntn), a, ntm, ntn, b_kc, vec, s);
  count_rows_form<WM, WN, TM, TN, BK>(form);
  return hipGetLastError();
}

// Split-K launch of the ntm x ntn tiles of `at` in S slices of whole K steps: block (tile, slice) stores its raw partial tile
// to `scratch`, splitk_reduce_kernel finishes C.  Whether to split and by how much is the caller's decision.
template <int WM, int WN, int TM, int TN, int BK>
void launch_split_k(RowsGemmArgs at, int ntm, int ntn, int S, long long ktot, float *scratch, bool b_kc, bool vec, hipStream_t s) {
  const long long kt = (ktot + BK - 1) / BK;
  at.kchunk = (int)(((kt + S - 1) / S) * BK);
  at.ksplit = (int)((ktot + at.kchunk - 1) / at.kchunk);
  at.partial = scratch;
  note_rows_slices(at.ksplit);
  launch_rows_kernel<WM, WN, TM, TN, BK>(dim3(ntm * ntn * at.ksplit), at, ntm, ntn, b_kc, vec, s);
  const long long total = (long long)at.M * at.N;
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)std::min<long long>((total + 255) / 256, 2048)), dim3(256), 0, s, at);
}

template <int WM, int WN, int TM, int TN, int BK>
int rows_slots_per_cu(int prec) {
  int per_cu = (WM * TM == 4 && WN * TN == 4 && BK == 16 && prec == 0) ? 3 : 2;
  if (prec == 3 && WN * TN == 5) per_cu = 1;
  if (WM * TM == 2 && prec == 0) per_cu = 4;  // 64-row tiles (27 KiB of LDS, 32 accumulator registers)
  return per_cu;
}
template <int WM, int WN, int TM, int TN, int BK>
int rows_slots(int prec) {  // resident blocks on the chip for this tile variant
  // Blocks per CU are MEASURED (tools/residency_probe.py: time of a plain launch steps up when one more tile needs one
  // more round), not queried: hipOccupancyMaxActiveBlocksPerMultiprocessor answers 3 for the 128x160 tile (168
  // registers, 46 KiB LDS) where the steps sit at 513 and 1025 tiles, i.e. 2 per CU (MI355X_MICROARCH.md warns that the
  // query can over-report).  128x128 BK 32: 2 (73.7 KiB LDS); 128x128 BK 16: 3 (41 KiB, 154 registers; steps at 513,
  // 769, 1025); 128x160: 2.
  // Split-bf16 variants are LDS-bound: 2 planes 128x128 BK 32 80 KiB (2), 128x160 BK 16 54 KiB (2); 3 planes 128x128
  // BK 16 72 KiB (2), 128x160 BK 16 81 KiB (1).
  return rows_slots_per_cu<WM, WN, TM, TN, BK>(prec) * device_cus();
}

// scratch for split-K partial tiles: allocated once, on first use (64 MiB covers slots x BM x BN floats)
constexpr size_t kScratchDefaultBytes = 64u << 20;
float *splitk_scratch(size_t *bytes) {
  if (g_scratch_override) {
    *bytes = g_scratch_override_bytes;
    return g_scratch_override;
  }
  static float *buf = nullptr;
  static bool tried = false;
  if (!tried) {
    tried = true;
    if (hipMalloc((void **)&buf, kScratchDefaultBytes) != hipSuccess) buf = nullptr;
    (void)hipGetLastError();
  }
  *bytes = kScratchDefaultBytes;
  return buf;
}

template <int WM, int WN, int TM, int TN, int BK>
hipError_t launch_rows_balanced(const RowsGemmArgs &a, bool b_kc, bool vec, int cls, double flops, hipStream_t s) {
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  const int ntm = (a.M + BM - 1) / BM, ntn = (a.N + BN - 1) / BN;
  int slots = rows_slots<WM, WN, TM, TN, BK>((b_kc && vec) ? a.prec : 0);
  if constexpr (kRingTile<WM, WN, TM, TN>) {
    if (ring_applies(a, b_kc, vec, BN)) slots = rows_gemm_ring_slots(BN);
  }
  const int tiles = ntm * ntn;
  const int q = tiles / slots, r = tiles % slots;
  const bool stats = a.colstats != nullptr;  // (rows_gemm() leaves it set only for the exact-f32 128 x 128 tile)
  const auto [ktot, k4] = k_range(a);
  // All blocks run equally long, so q*slots + r tiles cost q+1 rounds.  When the last round would be less than
  // half full, finish the last rows with a split-K launch that spreads them over every CU instead.
  const int main_mt = (q * slots) / ntn;  // full tile rows handled by the plain launch
  float *scratch = nullptr;
  size_t scratch_bytes = 0;
  // A handful of tiles with a long reduction (the R x D products of the natural-gradient state, P = M M^T of the
  // orthonormal constraint): one block per tile would crawl through K at load latency on a few CUs, so split K
  // over the idle ones.
  // (and a launch of more than slots / 4 but fewer than `slots` tiles -- one partly filled round: 188 row tiles of the 1500 x 16 shard's
  // full-rate .linear layers leave 68 of 256 CUs idle for the whole launch -- splits K by the factor S that fills whole rounds of CUs
  // best, ceil(tiles S / CUs) / S smallest: 188 tiles -> S = 4, 752 quarter tiles = 2.94 rounds of 256 instead of 4 quarters on 188 CUs)
  int S_partial = 0;
  if (!stats && q == 0 && tiles * 4 > slots && k4 && options().splitk_partial_round) {
    const int cus = device_cus();
    const long long kt = (ktot + BK - 1) / BK;
    double best = (double)((tiles + cus - 1) / cus);  // S = 1
    for (int S = 2; S <= 8; S++) {
      if (kt / S < 24) break;  // at least 24 K steps per slice
      const double cost = (double)(((long long)tiles * S + cus - 1) / cus) / S + 0.02 * S;  // (+ the partial tiles' round trip)
      if (cost < best - 1e-9) {
        best = cost;
        S_partial = S;
      }
    }
  }
  if (!stats && (tiles * 4 <= slots || S_partial >= 2) && k4 && ktot >= 16 * BK && (scratch = splitk_scratch(&scratch_bytes))) {
    const long long kt = (ktot + BK - 1) / BK;
    int S = S_partial >= 2 ? S_partial : slots / tiles;
    if (S_partial < 2 && options().splitk_per_cu == 1) S = std::max(2, device_cus() / tiles);  // (one slice per CU: half the partial tiles)
    if (S > kt / 4) S = (int)(kt / 4);
    const size_t need = sizeof(float) * (size_t)S * a.M * ((a.N + 3) & ~3);
    if (S >= 2 && need <= scratch_bytes) {
      ProfScope ps(cls, flops, s);
      launch_split_k<WM, WN, TM, TN, BK>(a, ntm, ntn, S, ktot, scratch, b_kc, vec, s);
      count_rows_form<WM, WN, TM, TN, BK>(S_partial >= 2 ? kFormPartialS2 + S_partial - 2 : kFormSplitK);
      return hipGetLastError();
    }
  }
  if (q >= 1 && r > 0 && 2 * r <= slots && main_mt > 0 && main_mt < ntm && k4 && ktot >= 8 * BK && (scratch = splitk_scratch(&scratch_bytes))) {
    const int m_main = main_mt * BM;
    RowsGemmArgs am = a;
    am.M = m_main;
    // column statistics: the main launch writes one partial row per row tile, the tail rows follow as the chunks of a
    // column-reduction pass over the finished C (split-K tail) or as the tail launch's own row tiles (plain tail)
    const int tail_rows = a.M - m_main;
    const long long kt_tail = (ktot + BK - 1) / BK;
    const int tail_tiles0 = ((tail_rows + BM - 1) / BM) * ntn;
    int S_tail = slots / tail_tiles0;
    if (S_tail > kt_tail / 2) S_tail = (int)(kt_tail / 2);
    const bool tail_split = S_tail >= 2 && sizeof(float) * (size_t)S_tail * tail_rows * ((a.N + 3) & ~3) <= scratch_bytes;
    ColReducePlan tail_plan = colreduce_plan(tail_rows, a.N);
    if (stats) {
      am.colstats_stride = main_mt + (tail_split ? tail_plan.chunks : (tail_rows + BM - 1) / BM);
      *a.colstats_rows = am.colstats_stride;
    }
    {
      ProfScope ps(cls, flops * m_main / a.M, s);
      hipError_t e = launch_rows<WM, WN, TM, TN, BK>(am, b_kc, vec, s);
      if (e != hipSuccess) return e;
    }
    RowsGemmArgs at = a;
    at.M = a.M - m_main;
    at.A = a.A + (long long)m_main * a.lda;
    at.C = a.C + (long long)m_main * a.ldc;
    for (int i = 0; i < at.nseg; i++) {
      at.seg[i].m_lo -= m_main;
      at.seg[i].m_hi -= m_main;
    }
    at.add_lo -= m_main;
    at.add_hi -= m_main;
    if (stats) {  // partial rows main_mt .. of the same array (the sums of squares sit colstats_stride rows further in both views)
      at.colstats = a.colstats + (long long)main_mt * a.N;
      at.colstats_stride = am.colstats_stride;
    }
    if (tail_split) {
      {
        ProfScope ps(cls, flops * at.M / a.M, s);
        launch_split_k<WM, WN, TM, TN, BK>(at, (at.M + BM - 1) / BM, ntn, S_tail, ktot, scratch, b_kc, vec, s);
        count_rows_form<WM, WN, TM, TN, BK>(kFormMainSplitTail);
      }
      if (stats) {
        MatView ct{at.C, at.M, at.N, (int)at.ldc};
        hipError_t e = colreduce_partial_into(1, ct, ct, tail_plan.chunks, tail_plan.rows_per_chunk, am.colstats_stride, at.colstats, s);
        if (e != hipSuccess) return e;
      }
      return hipGetLastError();
    }
    // tail too small to split: plain launch of the remaining rows
    ProfScope ps(cls, flops * at.M / a.M, s);
    const hipError_t e = launch_rows<WM, WN, TM, TN, BK>(at, b_kc, vec, s);
    count_rows_form<WM, WN, TM, TN, BK>(kFormMainPlainTail);
    return e;
  }
  ProfScope ps(cls, flops, s);
  if (stats) {
    RowsGemmArgs as = a;
    as.colstats_stride = ntm;
    *a.colstats_rows = ntm;
    return launch_rows<WM, WN, TM, TN, BK>(as, b_kc, vec, s);
  }
  return launch_rows<WM, WN, TM, TN, BK>(a, b_kc, vec, s);
}

// A launch with p.sumsq: one column tile, block b owns rows [BM b, BM b + BM).  Few row blocks and a long reduction (the
// natural-gradient H = X W^T of a small minibatch: 30 blocks for 256 CUs, each crawling through K at load latency): split K
// over the idle CUs; every (block, slice) then writes the sum of squares of its own slice.
template <int WM, int WN, int TM, int TN, int BK>
hipError_t launch_rows_sumsq(const RowsGemmArgs &a, bool b_kc, bool vec, hipStream_t s) {
  constexpr int BM = WM * TM * 32;
  const int tiles = (a.M + BM - 1) / BM, slots = rows_slots<WM, WN, TM, TN, BK>(0);
  const auto [ktot, k4] = k_range(a);
  float *scratch = nullptr;
  size_t scratch_bytes = 0;
  if (tiles * 4 <= slots && k4 && ktot >= 16 * BK && (scratch = splitk_scratch(&scratch_bytes))) {
    const long long kt = (ktot + BK - 1) / BK;
    int S = slots / tiles;
    if (S > kt / 4) S = (int)(kt / 4);
    if (S > 16) S = 16;
    const size_t need = sizeof(float) * (size_t)S * a.M * ((a.N + 3) & ~3);
    if (S >= 2 && need <= scratch_bytes && tiles * S <= a.sumsq_cap) {
      launch_split_k<WM, WN, TM, TN, BK>(a, tiles, 1, S, ktot, scratch, b_kc, vec, s);
      count_rows_form<WM, WN, TM, TN, BK>(kFormSumsqSplitK);
      return hipGetLastError();
    }
  }
  return launch_rows<WM, WN, TM, TN, BK>(a, b_kc, vec, s, kFormSumsqPlain);
}

// A launch with the inference epilogue (RowsGemmArgs::col_scale ...): one plain launch of rows_gemm_post_kernel -- no K split (its
// partial tiles would need the stage in the reduce kernel as well), no LDS-DMA ring, exact f32.
template <int WM, int WN, int TM, int TN, int BK>
hipError_t launch_rows_post(const RowsGemmArgs &a, bool vec, int cls, double flops, hipStream_t s) {
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  const int ntm = (a.M + BM - 1) / BM, ntn = (a.N + BN - 1) / BN;
  constexpr size_t lds = rows_lds_bytes<BM, BN, BK>(true);
  static const bool opted = opt_in_lds(rows_gemm_post_kernel<WM, WN, TM, TN, BK, 4>, lds) && opt_in_lds(rows_gemm_post_kernel<WM, WN, TM, TN, BK, 1>, lds);
  (void)opted;
  ProfScope ps(cls, flops, s);
  note_launch(0, vec);
  count_rows_form<WM, WN, TM, TN, BK>(kFormPost);
  if (vec) hipLaunchKernelGGL((rows_gemm_post_kernel<WM, WN, TM, TN, BK, 4>), dim3(ntm * ntn), dim3(256), lds, s, a, ntm, ntn);
  else hipLaunchKernelGGL((rows_gemm_post_kernel<WM, WN, TM, TN, BK, 1>), dim3(ntm * ntn), dim3(256), lds, s, a, ntm, ntn);
  return hipGetLastError();
}

// floor division / modulus for element offsets that may be negative (row shifts of the backward-data gather)
inline long long floordiv(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// The rows GEMM on the pre-split plane kernels (planes_gemm.hip) when the caller's hint describes these operands.  Everything is
// checked against the hint (base pointers, leading dimensions, 16-column alignment of the K segments, zero rows wherever a segment's
// view leaves [m_lo, m_hi)); false = not applicable, nothing launched.
bool planes_try_rows(const RowsGemmArgs &a, bool b_kc, int np, double flops, hipStream_t s, hipError_t *err) {
  const PlanesOperand *ha = planes_hint_a(), *hb = planes_hint_b();
  if (!ha || !hb || ha->np != np || hb->np != np || !ha->P || a.sumsq || a.ksplit > 1 || a.nseg > 16) return false;
  // tap coefficients: only when they are exactly the vector folded into the weight planes, segment s = tap s (then the product needs none)
  if (ha->coef || (a.coef == nullptr) != (hb->coef == nullptr)) return false;
  long long coef_t0 = 0;  // segment s carries the coefficient of tap coef_t0 + s: the planes must hold exactly that tap there
  if (a.coef) {
    coef_t0 = a.coef - hb->coef;
    if (coef_t0 < 0 || coef_t0 >= 16 || hb->coef_period <= 0) return false;
  }
  if (a.lda != ha->ld || a.A < ha->base || (a.A - ha->base) % ha->ld != 0) return false;
  const long long arow0 = (a.A - ha->base) / ha->ld;
  const int BM = planes_gemm_tile_rows(a.N), BN = planes_gemm_tile_cols(a.N);
  const long long m_pad = (long long)((a.M + BM - 1) / BM) * BM, n_pad = (long long)((a.N + BN - 1) / BN) * BN;
  PlanesGemmArgs g;
  memset(&g, 0, sizeof(g));
  g.np = np;
  g.A = ha->P; g.RA = ha->R; g.scale_a = ha->scale; g.scale_b = hb->scale;
  if (a.ldb != hb->ld || a.B < hb->base) return false;
  const long long boff0 = a.B - hb->base;
  if (b_kc) {
    if (!hb->P) return false;
    g.B = hb->P; g.RB = hb->R;
  } else {
    if (!hb->PT) return false;
    g.B = hb->PT; g.RB = hb->Rt;
  }
  for (int i = 0; i < a.nseg; i++) {
    const GemmSeg &sg = a.seg[i];
    // A_s[m][k] = base[(arow0 + shift + m) * ld + c0 + k]
    const long long shift = floordiv(sg.a_off, ha->ld), c0 = sg.a_off - shift * ha->ld;
    if (c0 % 16 != 0 || c0 + sg.klen > ha->cols || sg.klen <= 0) return false;
    const long long first = arow0 + shift;  // matrix row of output row 0
    const int lo = sg.m_lo > 0 ? sg.m_lo : 0, hi = sg.m_hi < a.M ? sg.m_hi : a.M;
    if (hi <= lo) return false;
    if (first + lo < 0 || first + hi > ha->rows) return false;       // rows that count must be the matrix's
    if (lo > 0 && first + lo != 0) return false;                      // rows below m_lo must fall into the lead zeros ...
    if (hi < a.M && first + hi != ha->rows) return false;             // ... and rows from m_hi on into the tail zeros
    if (ha->lead + first < 0 || ha->lead + first + m_pad > ha->R) return false;
    g.seg[i].a_row = ha->lead + first;
    g.seg[i].a_kb0 = (int)(c0 / 16);
    g.seg[i].nkb = (sg.klen + 15) / 16;
    if (sg.klen % 16 != 0 && c0 + sg.klen != ha->cols) return false;  // a ragged K block is zero-padded only at the matrix's end
    const long long bo = boff0 + sg.b_off;
    if (b_kc) {  // B[n][k] at base[(brow + n) * ld + bc0 + k]: the row-major planes of the hinted matrix
      const long long brow = bo / hb->ld, bc0 = bo % hb->ld;
      if (bo < 0 || bc0 % 16 != 0 || bc0 + sg.klen > hb->cols || brow + a.N > hb->rows || brow + n_pad > hb->R) return false;
      if (sg.klen % 16 != 0 && bc0 + sg.klen != hb->cols) return false;
      if (a.coef && (bc0 % hb->coef_period != 0 || bc0 / hb->coef_period != coef_t0 + i || sg.klen > hb->coef_period)) return false;
      g.seg[i].b_row = brow;
      g.seg[i].b_kb0 = (int)(bc0 / 16);
    } else {     // B[k][n] at base[(krow + k) * ld + ncol + n]: the transposed planes (k = row of the hinted matrix)
      const long long krow = bo / hb->ld, ncol = bo % hb->ld;
      if (bo < 0 || krow % 16 != 0 || krow + sg.klen > hb->rows || ncol + a.N > hb->cols || ncol + n_pad > hb->Rt) return false;
      if (sg.klen % 16 != 0 && krow + sg.klen != hb->rows) return false;
      if (a.coef && (ncol % hb->coef_period != 0 || ncol / hb->coef_period != coef_t0 + i || a.N > hb->coef_period)) return false;
      g.seg[i].b_row = ncol;
      g.seg[i].b_kb0 = (int)(krow / 16);
    }
  }
  g.nseg = a.nseg;
  g.alt_seg_order = a.alt_seg_order && a.nseg == 2 && g.seg[0].nkb == g.seg[1].nkb && g.seg[0].a_kb0 == g.seg[1].a_kb0 && g.seg[0].a_row != g.seg[1].a_row;
  if (g.alt_seg_order && options().gemm_alt_taps == 2 && g.seg[0].nkb >= 24 && !a.coef) {
    // the two taps in chunks of a few K blocks, alternating: a row block's two reads (as tap 0 by one tile, as the other tap by that tile or its
    // neighbour -- 256-row tiles, 128-row shift) are then a chunk apart instead of half a launch
    const PlanesSeg s0 = g.seg[0], s1 = g.seg[1];
    const int nchunk = std::min(16, s0.nkb / 6), per = (s0.nkb + nchunk - 1) / nchunk;
    int n = 0;
    for (int c = 0; c < nchunk; c++) {
      const int k0 = c * per, kn = std::min(per, s0.nkb - k0);
      if (kn <= 0) break;
      for (const PlanesSeg *sp : {&s0, &s1}) {
        PlanesSeg q = *sp;
        q.a_kb0 += k0;
        q.b_kb0 += k0;
        q.nkb = kn;
        g.seg[n++] = q;
      }
    }
    g.nseg = n;
    g.alt_seg_order = 0;
    count_form(kPlanesAltChunked);
  }
  g.skip_coef = a.coef;
  g.C = a.C; g.ldc = a.ldc; g.M = a.M; g.N = a.N;
  g.bias = a.bias; g.init_mode = a.init_mode; g.relu = a.relu;
  g.add = a.add; g.ldadd = a.ldadd; g.add_scale = a.add_scale; g.add_lo = a.add_lo; g.add_hi = a.add_hi;
  ProfScope ps(BN == 160 ? 1 : 0, flops, s);
  g_planes_routed_rows++;
  // One block per CU, equal block durations: a launch of q * CUs + r tiles costs q + 1 rounds.  When the last round would be less than
  // half full, the whole rounds run as one launch and the r tail tiles as a second one that splits K over the idle CUs (slabs in the
  // split-K scratch, then the epilogue): 260 row tiles of the 1/3-rate .linear layers on 256 CUs = 1.02 rounds instead of 2.
  {
    const int cus = device_cus();
    g.M = a.M;
    g.N = a.N;
    const int BMl = planes_gemm_launch_tile_rows(g);  // (128-row tiles for short reductions: two blocks per CU)
    const int ntm = (a.M + BMl - 1) / BMl, ntn = (a.N + BN - 1) / BN, tiles = ntm * ntn, slots = cus * (BMl == 128 ? 2 : 1), q = tiles / slots, r = tiles % slots;
    int nkb = 0;
    for (int i = 0; i < g.nseg; i++) nkb += g.seg[i].nkb;
    const int main_mt = (q * slots) / ntn;  // whole row tiles inside the full rounds
    // BatchNorm statistics of the stored output from the epilogue (RowsGemmArgs::colstats): one partial row per row tile
    const bool stats = a.colstats && a.colstats_rows && g.init_mode != 0;
    if (stats) {
      g.colstats = a.colstats;
      g.colstats_stride = ntm;
      *a.colstats_rows = ntm;
    }
    size_t scratch_bytes = 0;
    float *scratch = nullptr;
    // (a long K range only: with K = 320 the round that is saved is as short as the tail's two extra launches)
    if (q >= 1 && r > 0 && 2 * r <= slots && main_mt > 0 && main_mt < ntm && nkb >= 48 && BMl == BM && (scratch = splitk_scratch(&scratch_bytes))) {
      const int m_main = main_mt * BM, tail_rows = a.M - m_main, tail_tiles = ((tail_rows + BM - 1) / BM) * ntn;
      int S = std::min(cus / tail_tiles, nkb / 4);
      const long long ldp = (a.N + 3) & ~3;
      if (S >= 2 && sizeof(float) * (size_t)S * tail_rows * ldp <= scratch_bytes) {
        PlanesGemmArgs gm = g;
        gm.M = m_main;
        const ColReducePlan tail_plan = colreduce_plan(tail_rows, a.N);
        if (stats) {  // the main launch's row tiles, then the chunks of a column-reduction pass over the finished tail rows
          gm.colstats_stride = main_mt + tail_plan.chunks;
          *a.colstats_rows = gm.colstats_stride;
        }
        *err = planes_gemm(gm, s);
        if (*err != hipSuccess) return true;
        PlanesGemmArgs gt = g;
        gt.colstats = nullptr;
        gt.M = tail_rows;
        gt.C = g.C + (long long)m_main * g.ldc;
        for (int i = 0; i < gt.nseg; i++) gt.seg[i].a_row += m_main;
        if (gt.add) {  // (addend rows are relative to the launch's first output row)
          gt.add_lo = g.add_lo - m_main;
          gt.add_hi = g.add_hi - m_main;
          gt.add = g.add;
        }
        const int kbps = (nkb + S - 1) / S;
        gt.ksplit = (nkb + kbps - 1) / kbps;
        gt.kb_per_split = kbps;
        gt.partial = scratch;
        gt.partial_stride = (long long)tail_rows * ldp;
        gt.ldp_m = ldp;
        gt.ldp_n = 1;
        count_form(gt.ksplit >= 2 ? kPlanesMainSplitTail : kPlanesMainPlainTail);
        if (gt.ksplit >= 2) {
          *err = planes_gemm(gt, s);
          if (*err == hipSuccess) *err = planes_splitk_finish(gt, s);
        } else {
          gt.ksplit = 0;
          gt.partial = nullptr;
          *err = planes_gemm(gt, s);  // (a K range too short to split: the tail as a plain launch)
        }
        if (stats && *err == hipSuccess) {
          MatView ct{gt.C, tail_rows, a.N, (int)gt.ldc};
          *err = colreduce_partial_into(1, ct, ct, tail_plan.chunks, tail_plan.rows_per_chunk, gm.colstats_stride, a.colstats + (long long)main_mt * a.N, s);
        }
        return true;
      }
    }
  }
  count_form(kPlanesPlain);
  *err = planes_gemm(g, s);
  return true;
}

}  // namespace

SplitKScratchOverride::SplitKScratchOverride(float *buf, size_t bytes) : prev_buf(g_scratch_override), prev_bytes(g_scratch_override_bytes) {
  g_scratch_override = buf;
  g_scratch_override_bytes = bytes;
}
SplitKScratchOverride::~SplitKScratchOverride() {
  g_scratch_override = prev_buf;
  g_scratch_override_bytes = prev_bytes;
}
GemmPrecisionScope::GemmPrecisionScope(int prec) : prev(g_gemm_prec) { g_gemm_prec = prec; }
GemmPrecisionScope::~GemmPrecisionScope() { g_gemm_prec = prev; }
int gemm_precision_default() { return g_gemm_prec; }
TransposedWeightsScope::TransposedWeightsScope(const float *w_base, const float *wt_base, long long n) : prev_w(g_tw_w), prev_wt(g_tw_wt), prev_n(g_tw_n) {
  g_tw_w = w_base;
  g_tw_wt = wt_base;
  g_tw_n = n;
}
TransposedWeightsScope::~TransposedWeightsScope() {
  g_tw_w = prev_w;
  g_tw_wt = prev_wt;
  g_tw_n = prev_n;
}
const float *transposed_weights(const float *W) {
  if (!g_tw_w || !g_tw_wt || W < g_tw_w || W >= g_tw_w + g_tw_n) return nullptr;
  return g_tw_wt + (W - g_tw_w);
}

hipError_t rows_gemm(const RowsGemmArgs &a_in, bool b_kc, hipStream_t s) {
  if (a_in.M <= 0 || a_in.N <= 0 || a_in.nseg <= 0) return hipSuccess;
  RowsGemmArgs a = a_in;
  a.c_vec = aligned16(a.C) && a.ldc % 4 == 0 && (a.init_mode != 1 || aligned16(a.bias)) && (!a.add || (aligned16(a.add) && a.ldadd % 4 == 0));
  const bool vec = operands_vec4(a);
  // N == 160 (the TDNN-F bottleneck) gets a 128x160 tile so no column is wasted
  const int waste128 = ((a.N + 127) / 128) * 128 - a.N, waste160 = ((a.N + 159) / 160) * 160 - a.N;
  const long long ktot = k_range(a).ktot;
  double flops = 0;
  for (int i = 0; i < a.nseg; i++) flops += 2.0 * usable_rows(a.seg[i], a.M) * a.N * a.seg[i].klen;
  if (prof_on()) {
    // algorithmic bytes, each operand element once: the distinct A rows the segments read (taps of one matrix are row
    // shifts of it, so they share rows), the B blocks, the C tile written (and read when it is added to), the addend
    double a_elems = 0, b_elems = 0;
    bool taps = true;  // all segments: same reduction length, A offsets whole rows apart -> one matrix, shifted
    for (int i = 1; i < a.nseg; i++)
      taps = taps && a.seg[i].klen == a.seg[0].klen && a.lda > 0 && (a.seg[i].a_off - a.seg[0].a_off) % a.lda == 0;
    if (taps) {
      long long lo = a.seg[0].a_off, hi = a.seg[0].a_off;
      for (int i = 1; i < a.nseg; i++) {
        lo = std::min(lo, a.seg[i].a_off);
        hi = std::max(hi, a.seg[i].a_off);
      }
      a_elems = ((double)a.M + (double)(hi - lo) / (double)a.lda) * a.seg[0].klen;
    }
    for (int i = 0; i < a.nseg; i++) {
      if (!taps) a_elems += (double)usable_rows(a.seg[i], a.M) * a.seg[i].klen;
      b_elems += (double)a.seg[i].klen * a.N;
    }
    double c_elems = (double)a.M * a.N * (a.init_mode == 0 ? 2.0 : 1.0);
    if (a.add) c_elems += (double)(std::min(a.add_hi, a.M) - std::max(a.add_lo, 0)) * a.N;
    prof_next_gemm(flops, 4.0 * (a_elems + b_elems + c_elems));
  }
  a.serial_epilogue = 0;
  // two taps of one matrix: alternate the order row tile by row tile (rows_gemm_kernel)
  a.alt_seg_order = options().gemm_alt_taps && is_two_tap_shift(a);
  if (rows_gemm_has_post(a)) {  // the inference epilogue: the tile choice below, its own kernels
    if (!b_kc || a.init_mode == 0 || a.sumsq || a.ksplit > 1 || (a.init_mode == 1 && !a.bias)) return hipErrorInvalidValue;
    a.prec = 0;
    a.colstats = nullptr;
    if (a.colstats_rows) *a.colstats_rows = 0;
    a.c_vec = a.c_vec && (!a.col_scale || aligned16(a.col_scale)) && (!a.col_offset || aligned16(a.col_offset));
    if (waste160 < waste128) return launch_rows_post<4, 1, 1, 5, 16>(a, vec, 1, flops, s);
    if ((long long)((a.M + 127) / 128) * ((a.N + 127) / 128) < 768) return launch_rows_post<2, 2, 1, 2, 16>(a, vec, 0, flops, s);
    if (ktot <= 512) return launch_rows_post<2, 2, 2, 2, 16>(a, vec, 0, flops, s);
    return launch_rows_post<2, 2, 2, 2, 32>(a, vec, 0, flops, s);
  }
  if (a.prec == 0) {
    a.prec = g_gemm_prec;
    // tests (option gemm_arith_test): the in-kernel split-bf16 kernels for calls outside any GemmPrecisionScope
    if (a.prec == 0 && (options().gemm_arith_test == 1 || options().gemm_arith_test == 3)) a.prec = options().gemm_arith_test;
  }
  if (a.prec == 2) a.prec = 0;  // 2 = exact f32 regardless of the default
  if (a.prec == 4 || (a.prec == 3 && options().planes)) {  // pre-split planes (f16x3 / bf16x6) when the caller hinted them for these operands
    hipError_t pe = hipSuccess;
    if (planes_try_rows(a, b_kc, a.prec == 4 ? 2 : 3, flops, s, &pe)) return pe;
    if (a.prec == 4) a.prec = 0;  // no planes for this call: exact f32
  }
  if (!(b_kc && vec)) a.prec = 0;  // the split-bf16 kernels need a k-contiguous B and 16-byte alignment
  if (a.colstats_rows) *a.colstats_rows = 0;
  if (!a.colstats_rows || a.prec != 0 || a.sumsq || a.N <= 32 || waste160 < waste128 || a.ksplit > 1) a.colstats = nullptr;
  if (a.sumsq) {  // one column tile, no split-K tail: block b owns rows [128 b, 128 b + 128)
    if (a.N > 128) return hipErrorInvalidValue;
    a.sumsq_cap = rows_gemm_sumsq_blocks(a.M);
    ProfScope ps(0, flops, s);
    // (option ng_bk: 1 = K steps twice as long for these HBM-bound passes -- twice the bytes in flight per resident block)
    if (a.N <= 32) return (options().ng_bk & 1) ? launch_rows_sumsq<4, 1, 1, 1, 64>(a, b_kc, vec, s) : launch_rows_sumsq<4, 1, 1, 1, 32>(a, b_kc, vec, s);
    if (a.N <= 64 && a.N > 32 && (options().ng_bk & 8) == 0) return launch_rows_sumsq<4, 1, 1, 2, 32>(a, b_kc, vec, s);  // both taps' rank-20 products side by side (ng_stats.hip, P form)
    // long reductions (the rank-80 pass over the 6034-wide output derivative): the 128 x 128 tile, 48 idle columns and all, 1291 -> 1144 us;
    // short ones (160 columns) lose by it, 79 -> 106 (option ng_bk 4 forces it for both)
    if (a.N <= 96 && a.N > 64 && ((options().ng_bk & 4) || ktot >= 2048)) return launch_rows_sumsq<2, 2, 2, 2, 32>(a, b_kc, vec, s);
    if (a.N <= 96) return (options().ng_bk & 2) ? launch_rows_sumsq<4, 1, 1, 3, 32>(a, b_kc, vec, s) : launch_rows_sumsq<4, 1, 1, 3, 16>(a, b_kc, vec, s);  // rank-80 preconditioners: 96 of 96 columns, not 80 of 128
    return launch_rows_sumsq<2, 2, 2, 2, 32>(a, b_kc, vec, s);
  }
  // skinny outputs (the natural-gradient projections X W^T, rank <= 32): a 128x32 tile wastes no MFMA columns and
  // keeps three blocks per CU resident to pull the A operand at HBM rate
  if (a.N <= 32 && a.M >= 1024) {
    ProfScope ps(0, flops, s);
    return (options().ng_bk & 1) ? launch_rows<4, 1, 1, 1, 64>(a, b_kc, vec, s) : launch_rows<4, 1, 1, 1, 32>(a, b_kc, vec, s);
  }
  if (waste160 < waste128) return launch_rows_balanced<4, 1, 1, 5, 16>(a, b_kc, vec, 1, flops, s);
  {
    // short reductions (K <= 512: affine forward, linear backward, prefinal layers): BK 16 halves the LDS footprint,
    // three blocks per CU cover each other's prologue / epilogue (+6..13 % measured); long reductions keep BK 32
    // launches that leave most of the chip's block slots empty with 128 x 128 tiles (the recipes' minibatch: 3 200 rows) take
    // 64 x 128 tiles: twice the blocks, so the busiest CU carries 3 half tiles instead of 2 whole ones
    const long long tiles128 = (long long)((a.M + 127) / 128) * ((a.N + 127) / 128);
    const bool small = tiles128 < 768;  // measured at 150 x 64: 13.45 -> 13.28 ms per step; 1500 x 16 unchanged
    if (small && a.prec == 0 && !a.sumsq) return launch_rows_balanced<2, 2, 1, 2, 16>(a, b_kc, vec, 0, flops, s);
    if ((ktot <= 512 && a.prec == 0) || a.prec == 3) return launch_rows_balanced<2, 2, 2, 2, 16>(a, b_kc, vec, 0, flops, s);
  }
  return launch_rows_balanced<2, 2, 2, 2, 32>(a, b_kc, vec, 0, flops, s);
}

// ---- grouped launch of skinny statistics passes (rows_gemm_group_kernel)
struct RowsGemmGroup {
  std::vector<RowsGemmArgs> args;  // as uploaded
  std::vector<int> first;
  RowsGemmArgs *d_args = nullptr;
  int *d_first = nullptr;
  int capacity = 0;
};
void rows_gemm_group_destroy(RowsGemmGroup *g) {
  if (!g) return;
  if (g->d_args) hipFree(g->d_args);
  if (g->d_first) hipFree(g->d_first);
  delete g;
}
// what the group kernel takes: exact f32, one 32-column tile with the ||A||^2 by-product, k-contiguous B, 16-byte aligned operands
bool rows_gemm_group_ok(const RowsGemmArgs &a) {
  if (a.M <= 0 || a.N <= 0 || a.N > 32 || !a.sumsq || a.nseg <= 0 || a.ksplit > 1 || a.colstats || a.add) return false;
  return operands_vec4(a);
}
hipError_t rows_gemm_group(const std::vector<RowsGemmArgs> &calls, RowsGemmGroup **cache, hipStream_t s) {
  if (calls.empty()) return hipSuccess;
  if (!*cache) *cache = new RowsGemmGroup();
  RowsGemmGroup &g = **cache;
  std::vector<RowsGemmArgs> prep(calls.size());
  std::vector<int> first(calls.size() + 1, 0);
  double flops = 0, bytes = 0;
  for (size_t i = 0; i < calls.size(); i++) {
    RowsGemmArgs a = calls[i];
    if (!rows_gemm_group_ok(a)) return hipErrorInvalidValue;
    a.c_vec = aligned16(a.C) && a.ldc % 4 == 0 && (a.init_mode != 1 || aligned16(a.bias));
    a.sumsq_cap = rows_gemm_sumsq_blocks(a.M);
    a.serial_epilogue = 0;
    a.ksplit = 0;
    a.partial = nullptr;
    a.prec = 0;
    a.colstats = nullptr;
    a.colstats_rows = nullptr;
    a.alt_seg_order = options().gemm_alt_taps && is_two_tap_shift(a);
    prep[i] = a;
    first[i + 1] = first[i] + (a.M + 127) / 128;
    const double kt = (double)k_range(a).ktot;
    flops += 2.0 * a.M * a.N * kt;
    bytes += 4.0 * ((double)a.M * kt + kt * a.N + (double)a.M * a.N);
  }
  const bool same = g.args.size() == prep.size() && memcmp(g.args.data(), prep.data(), sizeof(RowsGemmArgs) * prep.size()) == 0 && g.first == first;
  if (!same) {  // (fixed shapes and buffers: uploaded once; the copy is ordered on the launch's stream)
    if (g.capacity < (int)prep.size()) {
      if (g.d_args) hipFree(g.d_args);
      if (g.d_first) hipFree(g.d_first);
      hipError_t e = hipMalloc((void **)&g.d_args, sizeof(RowsGemmArgs) * prep.size());
      if (e != hipSuccess) return e;
      e = hipMalloc((void **)&g.d_first, sizeof(int) * (prep.size() + 1));
      if (e != hipSuccess) return e;
      g.capacity = (int)prep.size();
    }
    g.args = prep;
    g.first = first;
    hipError_t e = hipMemcpyAsync(g.d_args, g.args.data(), sizeof(RowsGemmArgs) * prep.size(), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(g.d_first, g.first.data(), sizeof(int) * first.size(), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
  }
  constexpr size_t lds = rows_lds_bytes<128, 32, 32>(true);
  ProfGemmRange prof(3, flops, bytes, s);
  RowsGemmTasks t{g.d_args, g.d_first, (int)prep.size()};
  note_launch(0, true);  // (rows_gemm_group_ok: 16-byte aligned operands only)
  count_rows_form<4, 1, 1, 1, 32>(kFormGrouped);
  hipLaunchKernelGGL((rows_gemm_group_kernel<4, 1, 1, 1, 32, true, 4>), dim3(first.back()), dim3(256), lds, s, t);
  return hipGetLastError();
}

}  // namespace tdnnf
