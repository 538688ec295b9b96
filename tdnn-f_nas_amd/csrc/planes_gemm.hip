// planes_gemm.hip -- f32-equivalent GEMMs on the 16-bit matrix cores from operands PRE-SPLIT into 16-bit planes in HBM: the host side of
// the GEMM (kernels: planes_gemm_kernels.h; operand preparation: planes_split.hip; C ABI: abi_planes.hip).
//
// Two arithmetics (planes_gemm.h):
//   np = 3 "bf16x6": a = a0 + a1 + a2 (three bf16 planes, 24 mantissa bits), a.b ~ the six products a_i b_j with i + j <= 2: 6/16 of
//     the f32 MFMA's cycles, 6 bytes per operand element.
//   np = 2 "f16x3":  a s = h + l with s a power of two taken from the operand's Frobenius norm (|x| <= ||X||_F, so s ||X||_F <= 65504
//     means NO element can overflow, whatever the data), two f16 planes (11 + 11 bits and the sign of the remainder); a.b ~ h h' + h l' +
//     l h': 3/16 of the f32 MFMA's cycles and 4 bytes per operand element -- what an f32 operand costs.  Norm-wise the error sits below
//     the exact-f32 kernel's own summation error (tests/test_gpu_planes_gemm.py, against float64): an element that is small against
//     its matrix's rms loses relative precision (its low plane becomes subnormal: absolute error <= 2^-25 of the scaled value 1), which a
//     product that sums thousands of typical elements does not see.
// The round-2 kernels (rows_gemm_kernels.h, rows_gemm_x3_kernel) split f32 operands when a staged tile goes to LDS and wait for exactly that
// path.  Here the split happens ONCE per operand, in a pass of its own (planes_split_kernels.h), into a layout made for the consumer.
//
// Reference semantics: the GEMMs of TdnnComponent::Propagate / Backprop / UpdateSimple (/root/reference/src/nnet3/nnet-tdnn-component.cc:302-324,
// :378-411, :452) with K-segments = taps (row-shifted views of one matrix), as rows_gemm() / wgrad().
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "planes_gemm.h"
#include "planes_gemm_kernels.h"

namespace tdnnf {

// ------------------------------------------------------------------------------------------------------ routing state
long long g_planes_routed_rows = 0, g_planes_routed_wgrad = 0;
static thread_local const PlanesOperand *g_hint_a = nullptr, *g_hint_b = nullptr;
PlanesHintScope::PlanesHintScope(const PlanesOperand *a, const PlanesOperand *b) : prev_a(g_hint_a), prev_b(g_hint_b) {
  g_hint_a = a;
  g_hint_b = b;
}
PlanesHintScope::~PlanesHintScope() {
  g_hint_a = prev_a;
  g_hint_b = prev_b;
}
const PlanesOperand *planes_hint_a() { return g_hint_a; }
const PlanesOperand *planes_hint_b() { return g_hint_b; }

// ------------------------------------------------------------------------------------------------------ the tile choice
int planes_gemm_tile_rows(int N) { return 256; }
int planes_gemm_tile_cols(int N) {
  const int w128 = ((N + 127) / 128) * 128 - N, w160 = ((N + 159) / 160) * 160 - N;
  if (w160 < w128) return 160;
  return N % 256 == 0 ? 256 : 128;  // (256 x 256 tiles: 2/3 of the 256 x 128 tile's operand bytes per flop)
}

// Short reductions (K = 320: the .affine forward and .linear backward-data GEMMs, 1536 columns out): a tile's 256 KB of output and
// its 20 K steps of loads both run at what ONE CU can move (~20-50 GB/s), one after the other when the CU holds a single block.
// 128 x 256 tiles of four waves take 72 KB of LDS: two blocks per CU, one storing while the other multiplies.
static bool small_row_tile(const PlanesGemmArgs &a) {
  if (a.np != 2 || a.a_rows_as_k || a.ntap > 1 || a.ksplit > 1 || a.M <= 4096 || planes_gemm_tile_cols(a.N) != 256) return false;
  int nkb = 0;
  for (int i = 0; i < a.nseg; i++) nkb += a.seg[i].nkb;
  return nkb <= 40;
}
int planes_gemm_launch_tile_rows(const PlanesGemmArgs &a) { return small_row_tile(a) ? 128 : 256; }

// ------------------------------------------------------------------------------------------------------ the launch
namespace {

template <int NP, int WM, int WN, int TM, int TN, bool ATR>
hipError_t launch(const PlanesGemmArgs &a, hipStream_t s) {
  typedef PlanesTile<NP, WM, WN, TM, TN> Tile;
  static bool attr_done = false;
  if (!attr_done) {
    hipError_t e = hipFuncSetAttribute((const void *)planes_gemm_kernel<NP, WM, WN, TM, TN, ATR>, hipFuncAttributeMaxDynamicSharedMemorySize, Tile::LDS_BYTES);
    if (e != hipSuccess) return e;
    attr_done = true;
  }
  const int ntm = (a.M + Tile::BM - 1) / Tile::BM, ntn = (a.N + Tile::BN - 1) / Tile::BN;
  const int nblk = ntm * ntn * (a.ntap > 1 ? a.ntap : 1) * (a.ksplit > 1 ? a.ksplit : 1);
  hipLaunchKernelGGL((planes_gemm_kernel<NP, WM, WN, TM, TN, ATR>), dim3(nblk), dim3(Tile::NT), (size_t)Tile::LDS_BYTES, s, a, ntm, ntn);
  return hipGetLastError();
}

// 160-wide tiles for the TDNN-F bottleneck, 256- / 128-wide otherwise; 8 waves (two per SIMD)
// Measured on MI355X for np = 3 (tools/planes_bench.py, f32-equivalent TFLOP/s; exact-f32 kernel of rows_gemm_kernels.h in brackets):
//   256 x 256 tile, 8 waves of 64 x 128:  N = 1536, K = 2 x 1536: 227 [130];  K = 2 x 160 (.affine forward): 162 [116]
//   256 x 160 tile, 8 waves of 32 x 160:  N = 160, K = 2 x 1536 (.linear forward): 151 [117]
//   256 x 128 tile, 4 x 2 waves of 64 x 64: 201 / 150.  Four waves of 64 rows x the tile's width: 194 / 121 (one wave per SIMD
//   leaves every LDS / barrier wait exposed); fragments double-buffered in registers: no gain, spills on the wide tiles.
template <int NP, bool ATR>
hipError_t launch_tile(const PlanesGemmArgs &a, hipStream_t s) {
  const int bn = planes_gemm_tile_cols(a.N);
  if (bn == 160) return launch<NP, 8, 1, 1, 5, ATR>(a, s);
  if (bn == 128) return launch<NP, 4, 2, 2, 2, ATR>(a, s);
  if constexpr (NP == 2 && !ATR)
    if (small_row_tile(a)) return launch<2, 2, 2, 2, 4, false>(a, s);
  return launch<NP, 4, 2, 2, 4, ATR>(a, s);
}

}  // namespace

hipError_t planes_gemm(const PlanesGemmArgs &a, hipStream_t s) {
  if (a.M <= 0 || a.N <= 0 || a.nseg <= 0) return hipSuccess;
  if (a.np != 2 && a.np != 3) return hipErrorInvalidValue;
  if (a.ntap > 1 && a.nseg != 1) return hipErrorInvalidValue;
  // a_rows_as_k: the A operand through transposing LDS reads (weight gradients from row-major planes)
  if (a.np == 3) return a.a_rows_as_k ? launch_tile<3, true>(a, s) : launch_tile<3, false>(a, s);
  return a.a_rows_as_k ? launch_tile<2, true>(a, s) : launch_tile<2, false>(a, s);
}

hipError_t planes_splitk_finish(const PlanesGemmArgs &a, hipStream_t s) {
  if (a.ksplit < 2 || a.ntap > 1 || a.ldp_n != 1 || !a.partial) return hipErrorInvalidValue;
  const long long total = (long long)a.M * a.N;
  hipLaunchKernelGGL(planes_splitk_finish_kernel, dim3((unsigned)std::min<long long>((total + 255) / 256, 2048)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace tdnnf
