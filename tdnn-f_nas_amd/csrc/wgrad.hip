// wgrad.hip -- host side of the weight gradient (gemm_f32.h): tile choice, the split of the rows into slabs that fill whole
// rounds of resident blocks, the router onto the pre-split plane kernels, the slab reduction.  Kernels: wgrad_kernels.h.
#include <algorithm>
#include <cstring>

#include "colreduce.h"
#include "common.h"
#include "device.h"
#include "gemm_f32.h"
#include "launch_forms.h"
#include "planes_gemm.h"
#include "wgrad_kernels.h"

namespace tdnnf {
namespace {

struct WgradPlan {
  int splits, rows_per_split, chunks, rows_per_chunk;
  size_t slab_floats, colsum_floats;
};

// tile shape of the weight-gradient kernel: 160-wide variants for the TDNN-F bottleneck dimension
struct WgradTile {
  int BM, BN, variant;  // variant 0: 128x128, 1: 160x128 (Do == 160-ish), 2: 128x160 (Di == 160-ish), 3: 32x128 (Do <= 32)
};
inline int waste_of(int n, int t) { return ((n + t - 1) / t) * t - n; }
WgradTile wgrad_tile(int Do, int Di, bool x3 = false, int N = 1 << 30) {
  if (Do <= 32) return {32, 128, 3};
  // few rows (the recipes' minibatch: 3 000 - 10 000): with the 160 x 128 / 128 x 160 tiles the reduction is so short that a block is mostly
  // prologue and a 80 KB partial tile (13 slabs of 256 rows: 25 MB of partials for 43 MB of operands); 64 x 64 tiles give six times the
  // tiles, so two or three slabs fill the chip (option wgrad_small)
  if (!x3 && options().wgrad_small && N <= options().wgrad_small) return {64, 64, 4};
  // split-bf16 arithmetic is not MFMA bound: the 160-wide tiles (92 KiB of LDS in bf16 planes, one block per CU) lose to
  // plain 128x128 tiles with a few wasted columns
  if (x3) return {128, 128, 0};  // J = H^T X of a rank <= 32 preconditioner: HBM-bound on X, no wasted MFMA rows
  if (waste_of(Do, 160) * 128 < waste_of(Do, 128) * 160 && waste_of(Do, 160) < waste_of(Do, 128)) return {160, 128, 1};
  if (waste_of(Di, 160) < waste_of(Di, 128)) return {128, 160, 2};
  return {128, 128, 0};
}

// dynamic LDS of a BM x BN tile: double-buffered dY and X tiles of 32 rows, padded by 4 floats (f32); NP bf16 planes per
// operand, K steps of 32 (NP 2) or 16 (NP 3) rows padded by 8 (split-bf16)
constexpr size_t wgrad_lds_bytes(int BM, int BN) { return sizeof(float) * 2 * (32 * (BM + 4) + 32 * (BN + 4)); }
template <int NP>
constexpr size_t wgrad_x3_lds_bytes(int BM, int BN) {
  return sizeof(__bf16) * 2 * NP * (size_t)(BM + BN) * (NP == 2 ? 40 : 24);
}

// resident wgrad blocks on the whole chip (blocks/CU from the occupancy API x CUs), queried once per variant
template <int WM, int WN, int TM, int TN>
int wgrad_slots_of() {
  static int slots = 0;
  if (slots == 0) {
    int occ = 2;
    const int cus = device_cus();
    constexpr size_t lds = wgrad_lds_bytes(WM * TM * 32, WN * TN * 32);
    opt_in_lds(wgrad_kernel<WM, WN, TM, TN, 4>, lds);
    opt_in_lds(wgrad_kernel<WM, WN, TM, TN, 1>, lds);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void *)wgrad_kernel<WM, WN, TM, TN, 4>, 256, lds) != hipSuccess || occ < 1) occ = 2;
    slots = std::min(occ * cus, 1024);  // wgrad_workspace_bytes() assumes at most 1024 resident blocks
    (void)hipGetLastError();
  }
  return slots;
}
int wgrad_slots(int variant) {
  if (variant == 4) return wgrad_slots_of<2, 2, 1, 1>();
  return variant == 1 ? wgrad_slots_of<1, 4, 5, 1>() : variant == 2 ? wgrad_slots_of<4, 1, 1, 5>() : variant == 3 ? wgrad_slots_of<1, 4, 1, 1>()
                                                                                                   : wgrad_slots_of<2, 2, 2, 2>();
}

inline int wgrad_min_rounds() { return 2; }

// Split the row (reduction) range so that tiles * splits fills whole rounds of resident blocks: every block
// runs equally long, so a grid of q*slots + r blocks costs q+1 rounds; we want r == 0 (just under a multiple).
WgradPlan wgrad_plan(int Do, int Di, int K, int N, int slots, int ktaps = 0, bool x3 = false) {
  if (ktaps > 0) { WgradPlan p2 = wgrad_plan(Do, Di, ktaps, N, slots, 0, x3); p2.slab_floats = (size_t)p2.splits * Do * K * Di; return p2; }
  WgradPlan pl;
  const WgradTile wt = wgrad_tile(Do, Di, x3, N);
  const int tiles = ((Do + wt.BM - 1) / wt.BM) * K * ((Di + wt.BN - 1) / wt.BN);
  const int max_splits = std::max(1, (N + 255) / 256);  // at least 256 rows per split
  int splits = 1;
  // at least two rounds of resident blocks: a launch sized for exactly one round runs two as soon as a few slots are taken by
  // another stream's kernels (the denominator, the natural-gradient side stream); with shorter blocks the stragglers cost half
  // (weight-gradient class 30.7 -> 29.1 ms per step)
  const int min_rounds = wgrad_min_rounds();
  for (int rounds = min_rounds; rounds <= std::max(4, min_rounds); rounds++) {
    splits = (rounds * slots) / tiles;
    if (splits >= 1 && (rounds * slots) / tiles * tiles >= rounds * slots * 3 / 4) break;  // >= 75 % of the round used
  }
  if (wt.variant == 4) splits = std::max(1, (2 * device_cus()) / tiles);  // two blocks per CU, long slabs
  if (splits < 1) splits = 1;
  if (splits > max_splits) splits = max_splits;
  int rps = (N + splits - 1) / splits;
  rps = ((rps + 31) / 32) * 32;
  pl.splits = (N + rps - 1) / rps;
  pl.rows_per_split = rps;
  pl.slab_floats = (size_t)pl.splits * Do * K * Di;
  pl.rows_per_chunk = 512;
  pl.chunks = (N + 511) / 512;
  pl.colsum_floats = (size_t)pl.chunks * Do;
  return pl;
}

// ---- kernel launches
struct WgradLaunch {  // what every kernel variant of one wgrad() call is launched with
  dim3 grid;
  int ntm, ntn, rows_per_split;
  float *partial;
  hipStream_t s;
};
// (wgrad_kernel takes the arguments with xcd_order set, wgrad_x3_kernel the caller's)
template <int WM, int WN, int TM, int TN, int TAG>
void launch_wgrad_tagged(const WgradLaunch &l, const WgradArgs &a_x, bool vec) {
  constexpr size_t lds = wgrad_lds_bytes(WM * TM * 32, WN * TN * 32);
  static const bool opted = opt_in_lds(wgrad_kernel<WM, WN, TM, TN, 4, TAG>, lds) && opt_in_lds(wgrad_kernel<WM, WN, TM, TN, 1, TAG>, lds);
  (void)opted;
  if (vec) hipLaunchKernelGGL((wgrad_kernel<WM, WN, TM, TN, 4, TAG>), l.grid, dim3(256), lds, l.s, a_x, l.ntm, l.ntn, l.rows_per_split, l.partial);
  else hipLaunchKernelGGL((wgrad_kernel<WM, WN, TM, TN, 1, TAG>), l.grid, dim3(256), lds, l.s, a_x, l.ntm, l.ntn, l.rows_per_split, l.partial);
}
template <int WM, int WN, int TM, int TN, int NP, int TAG>
void launch_wgrad_x3_tagged(const WgradLaunch &l, const WgradArgs &a) {
  constexpr size_t lds = wgrad_x3_lds_bytes<NP>(WM * TM * 32, WN * TN * 32);
  static const bool opted = opt_in_lds(wgrad_x3_kernel<WM, WN, TM, TN, NP, 1, TAG>, lds);
  (void)opted;
  hipLaunchKernelGGL((wgrad_x3_kernel<WM, WN, TM, TN, NP, 1, TAG>), l.grid, dim3(256), lds, l.s, a, l.ntm, l.ntn, l.rows_per_split, l.partial);
}
// every weight-gradient kernel launch goes through here.  planes: 0 exact f32, 2 / 3 split-bf16 with that many planes per operand
// where the tile has such kernels (X3: wgrad_tile() gives that arithmetic the 128x128 and 32x128 tiles only -- the 160-wide ones
// need 92 KiB of LDS); TAG 1: the launches booked to the natural-gradient class (as for rows_gemm_kernel)
template <int WM, int WN, int TM, int TN, bool X3>
void launch_wgrad(const WgradLaunch &l, const WgradArgs &a, const WgradArgs &a_x, bool vec, int planes) {
  const bool ng = prof_class_override() == 3;
  if constexpr (X3) {
    if (planes == 2) {
      if (ng) launch_wgrad_x3_tagged<WM, WN, TM, TN, 2, 1>(l, a);
      else launch_wgrad_x3_tagged<WM, WN, TM, TN, 2, 0>(l, a);
      return;
    }
    if (planes == 3) {
      if (ng) launch_wgrad_x3_tagged<WM, WN, TM, TN, 3, 1>(l, a);
      else launch_wgrad_x3_tagged<WM, WN, TM, TN, 3, 0>(l, a);
      return;
    }
  }
  if (ng) launch_wgrad_tagged<WM, WN, TM, TN, 1>(l, a_x, vec);
  else launch_wgrad_tagged<WM, WN, TM, TN, 0>(l, a_x, vec);
}

// sum of the split slabs into G (scaled, accumulated) and the bias column sums
hipError_t wgrad_finish(const WgradArgs &a, const float *partial, int splits, float *cs_partial, const float *ds1, const float *ds2, hipStream_t s) {
  hipError_t e;
  const long long total = (long long)a.Do * a.K * a.Di;
  int rb = (int)((total + 255) / 256);
  if (rb > 2048) rb = 2048;
  if (total <= 32768 && splits >= 8 && !ds1)
    hipLaunchKernelGGL(wgrad_reduce_small_kernel, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, s, partial, splits, a.Do, a.K * a.Di,
                       a.Di, a.coef, a.scale, a.G, a.ldg, a.accumulate);
  else
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(rb), dim3(256), 0, s, partial, splits, a.Do, a.K * a.Di, a.Di, a.coef,
                       a.scale, a.G, a.ldg, a.accumulate, ds1, ds2);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (a.bias_acc) {
    MatView dyv{const_cast<float *>(a.dY), a.N, a.Do, (int)a.lddy};
    e = colsum_add(dyv, a.scale, a.bias_acc, cs_partial, s);
  }
  return e;
}

// The weight gradient on the pre-split plane kernels: G = dY^T X_tap reduces over ROWS, so its operands are the transposed planes of
// dY and X (k = row); the taps are K-block offsets of X.  The operand with more columns gives the tile rows (Do < Di: the transposed
// product, stored through strides), the rows are split over the CUs into slabs that wgrad_finish() adds.  false = not applicable.
bool planes_try_wgrad(const WgradArgs &a, void *workspace, size_t workspace_bytes, int np, hipStream_t s, hipError_t *err) {
  const PlanesOperand *hy = planes_hint_a(), *hx = planes_hint_b();
  if (!hy || !hx || hy->np != np || hx->np != np) return false;
  if (a.row_stride != 1 || a.K > 16 || a.K < 1) return false;  // (tap coefficients: applied by the reduce, zero ones skipped in the kernel -- the compacted tap list is not needed)
  if (a.dY != hy->base || a.lddy != hy->ld || a.N != hy->rows || a.Do != hy->cols) return false;
  if (a.ldx != hx->ld || a.X < hx->base || (a.X - hx->base) % hx->ld != 0 || a.Di != hx->cols) return false;
  const long long xrow0 = (a.X - hx->base) / hx->ld;
  const int nkb = (a.N + 15) / 16;
  if (nkb < 16) return false;  // (too few rows to split over the chip: the f32 kernels)
  const bool normal = a.Do >= a.Di;  // the operand with more columns gives the tile rows
  const int M = normal ? a.Do : a.Di, Nn = normal ? a.Di : a.Do;
  const int BM = planes_gemm_tile_rows(Nn), BN = planes_gemm_tile_cols(Nn);
  const int ntm = (M + BM - 1) / BM, ntn = (Nn + BN - 1) / BN;
  const PlanesOperand *hm = normal ? hy : hx, *hn = normal ? hx : hy;  // operands giving the tile rows / columns
  if (!hn->PT || (long long)ntn * BN > hn->Rt) return false;
  for (int i = 0; i < a.K; i++)
    if (a.row_offsets[i] < 0 || a.row_offsets[i] % 16 != 0 || xrow0 + a.row_offsets[i] + a.N > hx->rows) return false;
  PlanesGemmArgs g;
  memset(&g, 0, sizeof(g));
  // the tile-row operand: its row-major planes through transposing LDS reads when they are there (no planes of the transpose needed
  // for the big matrix), else its transposed planes
  const long long m_first = hm->lead + (normal ? 0 : xrow0);  // first matrix row of the K range in the row-major buffer
  const bool atr = hm->P && m_first % 16 == 0 && (long long)ntm * (BM / 16) <= hm->kb_alloc && m_first + 16LL * nkb + (normal ? 0 : a.row_offsets[a.K - 1]) <= hm->R;
  if (atr) {
    g.A = hm->P; g.RA = hm->R; g.a_rows_as_k = 1;
    g.seg[0].a_row = m_first;
  } else {
    if (!hm->PT || (long long)ntm * BM > hm->Rt || (!normal && xrow0 % 16 != 0)) return false;
    g.A = hm->PT; g.RA = hm->Rt;
  }
  for (int i = 0; i < a.K; i++) {
    if (normal) g.tap_b_kb[i] = (int)((xrow0 + a.row_offsets[i]) / 16);
    else g.tap_a_kb[i] = (int)((a.row_offsets[i] + (atr ? 0 : xrow0)) / 16);
  }
  if (normal && (xrow0 % 16 != 0)) return false;
  const int cus = device_cus();
  const int tiles = ntm * ntn * a.K;
  const size_t slab = (size_t)a.Do * a.K * a.Di;
  int splits = std::max(2, (2 * cus) / tiles);  // two rounds of one block per CU
  splits = std::min(splits, nkb / 8);
  splits = (int)std::min<size_t>((size_t)splits, workspace_bytes / sizeof(float) / slab);
  if (splits < 2) return false;
  const int kbps = (nkb + splits - 1) / splits;
  splits = (nkb + kbps - 1) / kbps;
  if (splits < 2) return false;
  if (sizeof(float) * slab * splits + colreduce_bytes(a.N, a.Do) > workspace_bytes) return false;
  g.np = np;
  g.B = hn->PT; g.RB = hn->Rt;
  g.M = M; g.N = Nn;
  g.nseg = 1;
  g.seg[0].nkb = nkb;
  g.ntap = a.K;
  g.ksplit = splits; g.kb_per_split = kbps;
  g.partial = reinterpret_cast<float *>(workspace);
  g.partial_stride = (long long)slab;
  g.tap_off_p = a.Di;
  g.skip_coef = a.coef;
  if (normal) { g.ldp_m = (long long)a.K * a.Di; g.ldp_n = 1; }
  else { g.ldp_m = 1; g.ldp_n = (long long)a.K * a.Di; }
  {
    const double flops = 2.0 * a.N * a.Do * a.K * a.Di;
    if (prof_on())
      prof_next_gemm(flops, 4.0 * ((double)a.N * a.Do + ((double)a.N + a.row_offsets[a.K - 1] - a.row_offsets[0]) * a.Di + (double)a.Do * a.K * a.Di * (a.accumulate ? 2.0 : 1.0)));
    ProfScope ps(2, flops, s);
    *err = planes_gemm(g, s);
  }
  if (*err != hipSuccess) return true;
  *err = wgrad_finish(a, g.partial, splits, g.partial + slab * splits, hy->scale, hx->scale, s);
  g_planes_routed_wgrad++;
  count_form(kWgradPlanes);
  note_wgrad_slabs(splits);
  return true;
}

}  // namespace

size_t wgrad_workspace_bytes(int Do, int Di, int K, int N) {
  // sized for the largest split count any device can ask for (4 rounds of 8 blocks on 304 CUs), so the
  // answer does not depend on the GPU being present
  const WgradTile wt0 = wgrad_tile(Do, Di, false), wt1 = wgrad_tile(Do, Di, true);
  const int tiles = std::min(((Do + wt0.BM - 1) / wt0.BM) * ((Di + wt0.BN - 1) / wt0.BN),
                             ((Do + wt1.BM - 1) / wt1.BM) * ((Di + wt1.BN - 1) / wt1.BN));  // worst case: one active tap, either arithmetic
  // wgrad_plan picks one round when tiles <= slots/4 (splits = slots/tiles) and at most 4 rounds otherwise (< 16 splits);
  // slots <= 1024 on any gfx950 part
  // (with r = wgrad_min_rounds(): r rounds when tiles <= r slots / 4, i.e. splits = r slots / tiles, else < 16 splits)
  size_t max_splits = std::max<size_t>(1, std::min<size_t>((N + 255) / 256, std::max<size_t>((size_t)std::max(wgrad_min_rounds(), 4) * 1024 / tiles + 1, 16)));
  return sizeof(float) * (max_splits * Do * K * Di) + colreduce_bytes(N, Do) + 64;
}

hipError_t wgrad(const WgradArgs &a, void *workspace, size_t workspace_bytes, hipStream_t s) {
  if (a.N <= 0 || a.Do <= 0 || a.Di <= 0) return hipSuccess;
  if (workspace_bytes < wgrad_workspace_bytes(a.Do, a.Di, a.K, a.N)) return hipErrorInvalidValue;
  int planes = 0;  // 0: f32 MFMA; 2 / 3: split-bf16 with that many planes per operand
  {
    int prec = a.prec;
    if (prec == 0) {
      prec = gemm_precision_default();
      if (prec == 0 && (options().gemm_arith_test == 1 || options().gemm_arith_test == 3)) prec = options().gemm_arith_test;  // (tests: rows_gemm.hip)
    }
    if (prec == 4 || (prec == 3 && options().planes)) {  // pre-split planes when the caller hinted them for these operands
      hipError_t pe = hipSuccess;
      if (planes_try_wgrad(a, workspace, workspace_bytes, prec == 4 ? 2 : 3, s, &pe)) return pe;
    }
    planes = prec == 1 ? 2 : prec == 3 ? 3 : 0;
  }
  const bool use_x3 = planes != 0;
  const WgradTile wt = wgrad_tile(a.Do, a.Di, use_x3, a.N);
  const int ktaps = a.active && a.max_active > 0 && a.max_active < a.K ? a.max_active : a.K;
  WgradArgs a_x = a;
  a_x.xcd_order = ktaps > 1 ? 1 : 0;  // the taps of a tile side by side on one XCD
  WgradPlan pl = wgrad_plan(a.Do, a.Di, a.K, a.N, wgrad_slots(wt.variant), ktaps == a.K ? 0 : ktaps, use_x3);
  if (sizeof(float) * pl.slab_floats > workspace_bytes) return hipErrorInvalidValue;
  float *partial = reinterpret_cast<float *>(workspace);
  float *cs_partial = partial + pl.slab_floats;
  const bool vec = aligned16(a.dY) && aligned16(a.X) && a.lddy % 4 == 0 && a.ldx % 4 == 0;
  const int ntm = (a.Do + wt.BM - 1) / wt.BM, ntn = (a.Di + wt.BN - 1) / wt.BN;
  const WgradLaunch l{dim3(ntm * ktaps * ntn, pl.splits), ntm, ntn, pl.rows_per_split, partial, s};
  {
    ProfFlopsScale exact(ktaps != a.K ? 1.0 : prof_flops_scale());  // a compacted launch already counts only its taps
    const double flops = 2.0 * a.N * a.Do * ktaps * a.Di;
    if (prof_on()) {  // algorithmic bytes: dY once, the distinct input rows once, the gradient block written (and read)
      int lo = a.row_offsets[0], hi = a.row_offsets[0];
      for (int i = 1; i < a.K; i++) {
        lo = std::min(lo, a.row_offsets[i]);
        hi = std::max(hi, a.row_offsets[i]);
      }
      prof_next_gemm(flops, 4.0 * ((double)a.N * a.Do + std::min((double)a.N * ktaps, (double)a.N * a.row_stride + (hi - lo)) * a.Di +
                                   (double)a.Do * ktaps * a.Di * (a.accumulate ? 2.0 : 1.0)));
    }
    ProfScope ps(2, flops, s);
    count_form(kWgradFirst + wt.variant * kRowsAriths + (planes == 2 ? 1 : planes == 3 ? 2 : 0));
    note_wgrad_slabs(pl.splits);
    if (wt.variant == 4) launch_wgrad<2, 2, 1, 1, false>(l, a, a_x, vec, planes);
    else if (wt.variant == 1) launch_wgrad<1, 4, 5, 1, false>(l, a, a_x, vec, planes);
    else if (wt.variant == 2) launch_wgrad<4, 1, 1, 5, false>(l, a, a_x, vec, planes);
    else if (wt.variant == 3) launch_wgrad<1, 4, 1, 1, true>(l, a, a_x, vec, planes);
    else launch_wgrad<2, 2, 2, 2, true>(l, a, a_x, vec, planes);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return wgrad_finish(a, partial, pl.splits, cs_partial, nullptr, nullptr, s);
}

}  // namespace tdnnf
