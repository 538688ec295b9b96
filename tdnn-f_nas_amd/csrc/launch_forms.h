// launch_forms.h -- process-wide counters of the kernel and launch form the GEMM planners chose (tdnnf_gemm_launch_forms,
// include/tdnnf_hip.h) and of the forms of the fused BatchNorm / ReLU sweeps (tdnnf_fused_launch_forms).  Observation only: nothing reads them back into a decision, counting is one relaxed atomic add on the host.
#pragma once
#include <atomic>

namespace tdnnf {

// ---- rows GEMM (rows_gemm.hip): one counter per (tile, arithmetic, form)
enum RowsForm {
  kFormPlain,          // one rows_gemm_kernel launch over all tiles
  kFormRing,           // the same launch taken by the persistent ring (gemm_ring.hip)
  kFormSplitK,         // launch_rows_balanced: few tiles, long reduction -- every tile split over K
  kFormPartialS2,      // launch_rows_balanced: one partly filled round, K split by S = 2 .. 8 (kFormPartialS2 + S - 2)
  kFormPartialS8 = kFormPartialS2 + 6,
  kFormMainSplitTail,  // launch_rows_balanced: whole rounds (counted as plain / ring as well), then a split-K launch of the last rows
  kFormMainPlainTail,  // ... then a plain launch of the last rows (two plain / ring counts)
  kFormSumsqPlain,     // launch_rows_sumsq without / with the K split
  kFormSumsqSplitK,
  kFormPost,           // launch_rows_post (the inference epilogue)
  kFormGrouped,        // rows_gemm_group
  kRowsForms
};
constexpr int kRowsTiles = 9, kRowsAriths = 3;  // arithmetic 0 exact f32, 1 split-bf16 with two planes (bf16x3), 2 with three (bf16x6)

template <int WM, int WN, int TM, int TN, int BK>
constexpr int rows_tile_index() {
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  constexpr int t = (BM == 128 && BN == 32 && BK == 32) ? 0 : (BM == 128 && BN == 32 && BK == 64) ? 1 : (BM == 128 && BN == 64 && BK == 32) ? 2
                  : (BM == 128 && BN == 96 && BK == 16) ? 3 : (BM == 128 && BN == 96 && BK == 32) ? 4 : (BM == 128 && BN == 160 && BK == 16) ? 5
                  : (BM == 64 && BN == 128 && BK == 16) ? 6 : (BM == 128 && BN == 128 && BK == 16) ? 7 : (BM == 128 && BN == 128 && BK == 32) ? 8 : -1;
  static_assert(t >= 0, "a rows GEMM tile without a counter: add it here and to kRowsTileNames (launch_forms.hip)");
  return t;
}
constexpr int rows_form_index(int tile, int arith, int form) { return (tile * kRowsAriths + arith) * kRowsForms + form; }

// ---- the plane router (planes_try_rows) and the weight gradient (wgrad.hip) behind the rows GEMM's block
enum {
  kPlanesPlain = kRowsTiles * kRowsAriths * kRowsForms,
  kPlanesMainSplitTail,
  kPlanesMainPlainTail,  // (whole rounds, then a tail whose K range was too short to split)
  kWgradFirst,           // + variant (wgrad_tile: 0 .. 4) * kRowsAriths + arithmetic
  kWgradPlanes = kWgradFirst + 5 * kRowsAriths,  // planes_try_wgrad
  kWgradLastSlabs,       // not a count: the number of row slabs (`splits`) of the last weight gradient
  kRowsLastSlices,       // not a count: the number of K slices the last split-K launch of the rows GEMM ran with
  kRowsVec4Launches,     // rows GEMM kernel launches (ring and grouped included) that load 16 bytes at a time / float by float
  kRowsScalarLaunches,
  kPlanesAltChunked,     // plane router: calls whose two taps went in alternating chunks of K blocks (option gemm_alt_taps 2)
  kLaunchFormCounters
};

std::atomic<long long> *launch_form_counters();  // kLaunchFormCounters of them
inline void count_form(int index) { launch_form_counters()[index].fetch_add(1, std::memory_order_relaxed); }
inline void note_rows_slices(int ksplit) { launch_form_counters()[kRowsLastSlices].store(ksplit, std::memory_order_relaxed); }
inline void note_wgrad_slabs(int splits) { launch_form_counters()[kWgradLastSlabs].store(splits, std::memory_order_relaxed); }

// ---- the fused BatchNorm / ReLU sweeps (fused.hip): counters of their own (tdnnf_fused_launch_forms), one add per call of the host
// functions bn_apply_bypass / bn_relu_bwd for every property of the launch below
enum { kFusedVec4, kFusedScalar, kFusedPlanes, kFusedKinds };  // the kernel instance: 16-byte accesses, float by float, or vec4 with the f16 plane stores
constexpr int kFusedFlagSuper = 1, kFusedFlagMask = 2, kFusedFlagRev = 4;  // bn_apply_bypass: super-row view, dropout mask given, reversed walk
constexpr int kFusedNgFlagMask = 1, kFusedNgFlagPlanes = 2, kFusedNgFlagRev = 4;
enum FusedForm {
  kFusedBypassFirst,                                      // + kind * 8 + flags (kFusedFlag*)
  kFusedReduceFirst = kFusedBypassFirst + kFusedKinds * 8,  // + (scalar ? 2 : 0) + (ReLU statistics ? 1 : 0)
  kFusedFinalizeTrain = kFusedReduceFirst + 4,
  kFusedFinalizeTest,
  kFusedApplyFirst,                                       // + kind * 4 + (mask ? 1 : 0) + (reversed ? 2 : 0)
  kFusedApplyUnrolled = kFusedApplyFirst + kFusedKinds * 4,  // apply launches in which some row lane runs the 16-row unrolled loop ...
  kFusedApplyTail,                                        // ... and the 4-row tail loop
  kFusedApplyShortChunk,                                  // ... whose last chunk of rows is shorter than the others
  kFusedNgFirst,                                          // + (NT - 1) * 8 + flags (kFusedNgFlag*)
  kFusedNgPartialBlock = kFusedNgFirst + 3 * 8,           // apply-ng launches whose last 128-row block is partial / that have none
  kFusedNgFullBlocks,
  kFusedRepair,                                           // bn_relu_bwd calls with the self-repair term switched on
  kFusedFormCounters
};
std::atomic<long long> *fused_form_counters();  // kFusedFormCounters of them
inline void count_fused(int index) { fused_form_counters()[index].fetch_add(1, std::memory_order_relaxed); }

}  // namespace tdnnf
