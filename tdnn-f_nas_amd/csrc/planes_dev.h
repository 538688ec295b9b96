// planes_dev.h -- device-side types shared by the plane kernels (planes_split_kernels.h, planes_gemm_kernels.h): the MFMA vector types and
// Plane<NP>, which says for each arithmetic of planes_gemm.h what an element is, how an f32 value splits into NP of them and which MFMA
// multiplies them.
#pragma once
#include <hip/hip_runtime.h>

namespace tdnnf {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

template <int NP>
struct Plane;
template <>
struct Plane<3> {
  typedef __bf16 E;
  typedef bf16x8 V8;
  static __device__ __forceinline__ f32x16 mfma(V8 a, V8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ void split(float x, E (&p)[3]) {
    p[0] = (__bf16)x;
    float r = x - (float)p[0];
    p[1] = (__bf16)r;
    r -= (float)p[1];
    p[2] = (__bf16)r;
  }
};
template <>
struct Plane<2> {
  typedef _Float16 E;
  typedef f16x8 V8;
  static __device__ __forceinline__ f32x16 mfma(V8 a, V8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ void split(float x, E (&p)[2]) {  // x already scaled
    p[0] = (_Float16)x;
    p[1] = (_Float16)(x - (float)p[0]);
  }
};

}  // namespace
}  // namespace tdnnf
