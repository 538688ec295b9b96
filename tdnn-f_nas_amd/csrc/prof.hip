// prof.hip -- the event-timing registry behind tdnnf_profile_* (prof.h).
#include "prof.h"

#include <vector>

#include "tdnnf_hip.h"

namespace tdnnf {

struct ProfClass {
  const char *name;
  std::vector<hipEvent_t> ev;  // pairs
  size_t used = 0;
  double flops = 0;
  double bytes = 0;
};

namespace {

constexpr int kProfClasses = 8, kProfGemmClasses = 4;
constexpr size_t kProfMaxLaunches = 1 << 15;
ProfClass g_prof[kProfClasses] = {{"rows_gemm_f32_128x128"}, {"rows_gemm_f32_128x160"}, {"wgrad_f32"}, {"ng_skinny_gemm_f32"},
                                  {"bn_apply_bypass"}, {"bn_relu_bwd"}, {"denominator"}, {"planes_split"}};
bool g_prof_on = false;
int g_prof_override = -1;
double g_prof_flops_scale = 1.0;
double g_prof_next_flops = 0, g_prof_next_bytes = 0;

// the class a range of class `cls` in [lo, hi) is booked to; null: not timed
ProfClass *admit(int cls, int lo, int hi) {
  if (!g_prof_on || cls < lo || cls >= hi) return nullptr;
  ProfClass &p = g_prof[cls];
  return p.used + 2 > p.ev.size() ? nullptr : &p;
}

}  // namespace

bool prof_on() { return g_prof_on; }
int prof_class_override() { return g_prof_override; }
double prof_flops_scale() { return g_prof_flops_scale; }
void prof_next_gemm(double flops, double bytes) {
  g_prof_next_flops = flops;
  g_prof_next_bytes = bytes;
}

ProfRange::ProfRange(ProfClass *cls, double flops, double bytes, hipStream_t stream) : c(cls), s(stream) {
  if (!c) return;
  c->flops += flops;
  c->bytes += bytes;
  hipEventRecord(c->ev[c->used], s);
}
ProfRange::~ProfRange() {
  if (!c) return;
  hipEventRecord(c->ev[c->used + 1], s);
  c->used += 2;
}

// (a launch that covers a fraction of the GEMM's rows -- main + split-K tail -- gets that fraction of its bytes)
ProfScope::ProfScope(int cls, double flops, hipStream_t stream)
    : ProfRange(admit(g_prof_override >= 0 ? g_prof_override : cls, 0, kProfClasses), flops * g_prof_flops_scale,
                g_prof_next_flops > 0 ? g_prof_next_bytes * (flops / g_prof_next_flops) : 0.0, stream) {}
ProfHbmRange::ProfHbmRange(int cls, double bytes, hipStream_t stream) : ProfRange(admit(cls, kProfGemmClasses, kProfClasses), 0.0, bytes, stream) {}
ProfGemmRange::ProfGemmRange(int cls, double flops, double bytes, hipStream_t stream) : ProfRange(admit(cls, 0, kProfGemmClasses), flops, bytes, stream) {}

ProfClassOverride::ProfClassOverride(int cls) : prev(g_prof_override) { g_prof_override = cls; }
ProfClassOverride::~ProfClassOverride() { g_prof_override = prev; }
ProfFlopsScale::ProfFlopsScale(double f) : prev(g_prof_flops_scale) { g_prof_flops_scale = f; }
ProfFlopsScale::~ProfFlopsScale() { g_prof_flops_scale = prev; }

}  // namespace tdnnf

extern "C" {
int tdnnf_profile_enable(int on) {
  using namespace tdnnf;
  if (on) {
    for (auto &p : g_prof) {
      if (p.ev.empty()) {
        p.ev.resize(2 * kProfMaxLaunches);
        for (auto &e : p.ev)
          if (hipEventCreate(&e) != hipSuccess) return TDNNF_EHIP;
      }
      p.used = 0;
      p.flops = 0;
      p.bytes = 0;
    }
  }
  g_prof_on = on != 0;
  return TDNNF_OK;
}
int tdnnf_profile_read(int cls, double *launches, double *total_ms, double *total_flops) {
  using namespace tdnnf;
  if (cls < 0 || cls >= kProfClasses) return TDNNF_EINVAL;
  ProfClass &p = g_prof[cls];
  double ms = 0;
  for (size_t i = 0; i + 1 < p.used; i += 2) {
    if (hipEventSynchronize(p.ev[i + 1]) != hipSuccess) return TDNNF_EHIP;
    float t = 0;
    if (hipEventElapsedTime(&t, p.ev[i], p.ev[i + 1]) != hipSuccess) return TDNNF_EHIP;
    ms += t;
  }
  if (launches) *launches = (double)(p.used / 2);
  if (total_ms) *total_ms = ms;
  if (total_flops) *total_flops = p.flops;
  return TDNNF_OK;
}
int tdnnf_profile_read_bytes(int cls, double *algorithmic_bytes) {
  if (cls < 0 || cls >= tdnnf::kProfClasses || !algorithmic_bytes) return TDNNF_EINVAL;
  *algorithmic_bytes = tdnnf::g_prof[cls].bytes;
  return TDNNF_OK;
}
const char *tdnnf_profile_class_name(int cls) { return cls >= 0 && cls < tdnnf::kProfClasses ? tdnnf::g_prof[cls].name : ""; }
}
