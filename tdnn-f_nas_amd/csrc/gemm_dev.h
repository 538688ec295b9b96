// gemm_dev.h -- device helpers shared by the rows GEMM and weight-gradient kernels (rows_gemm_kernels.h, wgrad_kernels.h).
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

namespace tdnnf {

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

// 16 zero bytes: predicated-off float4 loads of the fast path read here instead of branching
__device__ float4 g_zero4 = {0.f, 0.f, 0.f, 0.f};
// (It has to stay a variable the host could write, in every file that includes this header.  Naming it inside a lambda, as the rows
// GEMM kernels do, makes it one; where kernels only name it directly (wgrad_kernels.h) the compiler would treat it as a constant of the
// translation unit, fold the loads and reach it without the GOT -- other code than the kernels that were measured.  A host function
// that names it settles it the same way everywhere.)
[[maybe_unused]] inline const void *zero4_symbol() { return &g_zero4; }

__device__ __forceinline__ float4 ld4(const float *p, bool v0, bool v1, bool v2, bool v3, bool vec) {
  float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
  if (vec && v3) {  // whole float4 in range (validity is monotone in the element index)
    r = *reinterpret_cast<const float4 *>(p);
  } else {
    if (v0) r.x = p[0];
    if (v1) r.y = p[1];
    if (v2) r.z = p[2];
    if (v3) r.w = p[3];
  }
  return r;
}

// compile-time loop: f(IntC<0>{}), f(IntC<1>{}), ... -- register arrays indexed by the counter stay in registers without
// depending on the loop unroller
template <int V>
struct IntC {
  static constexpr int value = V;
};
template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F &&f, std::integer_sequence<int, I...>) {
  (f(IntC<I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// x = pl[0] + pl[1] (+ pl[2]) + O(2^-8NP |x|): each plane is the bf16 rounding of what the planes above it left.
template <int NP>
__device__ __forceinline__ void split_bf16(const float4 v, bf16x4 (&pl)[NP]) {
  const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    float r = x[i];
#pragma unroll
    for (int q = 0; q < NP; q++) {
      const __bf16 h = (__bf16)r;
      pl[q][i] = h;
      r -= (float)h;
    }
  }
}

}  // namespace
}  // namespace tdnnf
