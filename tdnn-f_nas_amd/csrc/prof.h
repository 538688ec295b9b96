// prof.h -- optional event timing of the library's launches by class (tdnnf_profile_*, include/tdnnf_hip.h).
// Classes 0 .. 3 are GEMMs (0 rows_gemm 128x128, 1 rows_gemm 128x160, 2 wgrad, 3 natural-gradient skinny GEMMs) and carry
// algorithmic FLOPs and bytes; classes 4 .. 7 are HBM-bound passes (4 bn_apply_bypass, 5 bn_relu_bwd (both stages), 6 denominator
// (forward + backward recursions), 7 planes_split) and carry bytes: every operand element touched once.
#pragma once
#include <hip/hip_runtime.h>

namespace tdnnf {

struct ProfClass;  // prof.hip

bool prof_on();              // tdnnf_profile_enable
int prof_class_override();   // the class of the innermost ProfClassOverride alive, -1 without one
double prof_flops_scale();   // the factor of the innermost ProfFlopsScale alive, 1 without one
// algorithmic work of the whole GEMM the next ProfScope(s) belong to (rows_gemm / wgrad say so before they launch)
void prof_next_gemm(double flops, double bytes);

// An event pair on `stream` around the launches made while it is alive, and their work added to the class's totals; nothing
// while timing is off or once the class holds its maximum number of ranges.  Made through one of the three forms below.
class ProfRange {
 public:
  ProfRange(const ProfRange &) = delete;
  ProfRange &operator=(const ProfRange &) = delete;
  ~ProfRange();

 protected:
  ProfRange(ProfClass *cls, double flops, double bytes, hipStream_t stream);  // cls null: not timed

 private:
  ProfClass *c;
  hipStream_t s;
};

// One launch (or the main / tail part) of the GEMM announced by prof_next_gemm: booked to the ProfClassOverride's class when one is
// alive, else to `cls`; `flops` scaled by the ProfFlopsScale, and of the GEMM's bytes the share flops / (the GEMM's flops).
struct ProfScope : ProfRange {
  ProfScope(int cls, double flops, hipStream_t stream);
};
// An HBM-bound pass (classes 4 .. 7 only) with its algorithmic bytes.
struct ProfHbmRange : ProfRange {
  ProfHbmRange(int cls, double bytes, hipStream_t stream);
};
// ONE launch of a GEMM class (0 .. 3 only; ng_valu.hip, the grouped statistics passes: class 3) with its own work, as given.
struct ProfGemmRange : ProfRange {
  ProfGemmRange(int cls, double flops, double bytes, hipStream_t stream);
};

// Event-timing class of the ProfScope launches made while one of these is alive.
struct ProfClassOverride {
  int prev;
  explicit ProfClassOverride(int cls);
  ~ProfClassOverride();
};

// Scales the algorithmic FLOPs recorded for the ProfScope launches made while alive: the host cannot see device-side tap
// coefficients, so a caller that knows only `active` of K taps are non-zero (DARTS uniform-sample mode) says so.
struct ProfFlopsScale {
  double prev;
  explicit ProfFlopsScale(double f);
  ~ProfFlopsScale();
};

}  // namespace tdnnf
