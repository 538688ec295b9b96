// launch_forms.hip -- the counters of launch_forms.h and their C-ABI (tdnnf_gemm_launch_forms, tdnnf_gemm_launch_form_name,
// tdnnf_fused_launch_forms, tdnnf_fused_launch_form_name).
#include "launch_forms.h"

#include <stdio.h>

#include "common.h"

namespace tdnnf {

std::atomic<long long> *launch_form_counters() {
  static std::atomic<long long> counters[kLaunchFormCounters];  // (zero-initialised)
  return counters;
}

std::atomic<long long> *fused_form_counters() {
  static std::atomic<long long> counters[kFusedFormCounters];  // (zero-initialised)
  return counters;
}

namespace {
const char *const kFusedKindNames[kFusedKinds] = {"vec4", "scalar", "planes"};
const char *const kRowsTileNames[kRowsTiles] = {"128x32k32", "128x32k64", "128x64k32", "128x96k16", "128x96k32", "128x160k16", "64x128k16", "128x128k16", "128x128k32"};
const char *const kArithNames[kRowsAriths] = {"f32", "bf16x3", "bf16x6"};
const char *const kRowsFormNames[kRowsForms] = {"plain", "ring", "splitk", "partial_s2", "partial_s3", "partial_s4", "partial_s5", "partial_s6", "partial_s7", "partial_s8",
                                                "main_split_tail", "main_plain_tail", "sumsq_plain", "sumsq_splitk", "post", "grouped"};
const char *const kWgradTileNames[5] = {"128x128", "160x128", "128x160", "32x128", "64x64"};
}  // namespace

}  // namespace tdnnf

using namespace tdnnf;

extern "C" {

const char *tdnnf_gemm_launch_form_name(int index) {
  static thread_local char buf[64];
  if (index < 0 || index >= kLaunchFormCounters) return nullptr;
  if (index < kPlanesPlain) {
    const int form = index % kRowsForms, arith = (index / kRowsForms) % kRowsAriths, tile = index / (kRowsForms * kRowsAriths);
    snprintf(buf, sizeof(buf), "rows.%s.%s.%s", kRowsTileNames[tile], kArithNames[arith], kRowsFormNames[form]);
  } else if (index == kPlanesPlain) {
    snprintf(buf, sizeof(buf), "planes.plain");
  } else if (index == kPlanesMainSplitTail) {
    snprintf(buf, sizeof(buf), "planes.main_split_tail");
  } else if (index == kPlanesMainPlainTail) {
    snprintf(buf, sizeof(buf), "planes.main_plain_tail");
  } else if (index < kWgradPlanes) {
    const int i = index - kWgradFirst;
    snprintf(buf, sizeof(buf), "wgrad.%s.%s", kWgradTileNames[i / kRowsAriths], kArithNames[i % kRowsAriths]);
  } else if (index == kWgradPlanes) {
    snprintf(buf, sizeof(buf), "wgrad.planes");
  } else if (index == kWgradLastSlabs) {
    snprintf(buf, sizeof(buf), "wgrad.last_slabs");
  } else if (index == kRowsLastSlices) {
    snprintf(buf, sizeof(buf), "rows.last_slices");
  } else if (index == kRowsVec4Launches) {
    snprintf(buf, sizeof(buf), "rows.launches_vec4");
  } else if (index == kRowsScalarLaunches) {
    snprintf(buf, sizeof(buf), "rows.launches_scalar");
  } else {
    snprintf(buf, sizeof(buf), "planes.alt_chunked");
  }
  return buf;
}

int tdnnf_gemm_launch_forms(long long *counts, int capacity, int reset) {
  std::atomic<long long> *c = launch_form_counters();
  for (int i = 0; i < kLaunchFormCounters; i++) {
    if (counts && i < capacity) counts[i] = c[i].load(std::memory_order_relaxed);
    if (reset) c[i].store(0, std::memory_order_relaxed);
  }
  return kLaunchFormCounters;
}

const char *tdnnf_fused_launch_form_name(int index) {
  static thread_local char buf[64];
  if (index < 0 || index >= kFusedFormCounters) return nullptr;
  if (index < kFusedReduceFirst) {
    const int i = index - kFusedBypassFirst, f = i % 8;
    snprintf(buf, sizeof(buf), "apply_bypass.%s%s%s%s", kFusedKindNames[i / 8], f & kFusedFlagSuper ? ".super" : "", f & kFusedFlagMask ? ".mask" : "",
             f & kFusedFlagRev ? ".rev" : "");
  } else if (index < kFusedFinalizeTrain) {
    const int i = index - kFusedReduceFirst;
    snprintf(buf, sizeof(buf), "bwd.reduce.%s.%s", i & 2 ? "scalar" : "vec4", i & 1 ? "stats" : "nostats");
  } else if (index == kFusedFinalizeTrain) {
    snprintf(buf, sizeof(buf), "bwd.finalize.train");
  } else if (index == kFusedFinalizeTest) {
    snprintf(buf, sizeof(buf), "bwd.finalize.test");
  } else if (index < kFusedApplyUnrolled) {
    const int i = index - kFusedApplyFirst, f = i % 4;
    snprintf(buf, sizeof(buf), "bwd.apply.%s%s%s", kFusedKindNames[i / 4], f & 1 ? ".mask" : "", f & 2 ? ".rev" : "");
  } else if (index == kFusedApplyUnrolled) {
    snprintf(buf, sizeof(buf), "bwd.apply.rows_unrolled");
  } else if (index == kFusedApplyTail) {
    snprintf(buf, sizeof(buf), "bwd.apply.rows_tail");
  } else if (index == kFusedApplyShortChunk) {
    snprintf(buf, sizeof(buf), "bwd.apply.short_last_chunk");
  } else if (index < kFusedNgPartialBlock) {
    const int i = index - kFusedNgFirst, f = i % 8;
    snprintf(buf, sizeof(buf), "bwd.apply_ng.nt%d%s%s%s", i / 8 + 1, f & kFusedNgFlagMask ? ".mask" : "", f & kFusedNgFlagPlanes ? ".planes" : "",
             f & kFusedNgFlagRev ? ".rev" : "");
  } else if (index == kFusedNgPartialBlock) {
    snprintf(buf, sizeof(buf), "bwd.apply_ng.partial_block");
  } else if (index == kFusedNgFullBlocks) {
    snprintf(buf, sizeof(buf), "bwd.apply_ng.full_blocks");
  } else {
    snprintf(buf, sizeof(buf), "bwd.repair");
  }
  return buf;
}

int tdnnf_fused_launch_forms(long long *counts, int capacity, int reset) {
  std::atomic<long long> *c = fused_form_counters();
  for (int i = 0; i < kFusedFormCounters; i++) {
    if (counts && i < capacity) counts[i] = c[i].load(std::memory_order_relaxed);
    if (reset) c[i].store(0, std::memory_order_relaxed);
  }
  return kFusedFormCounters;
}

}  // extern "C"
