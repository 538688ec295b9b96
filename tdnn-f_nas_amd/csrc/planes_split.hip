// planes_split.hip -- host side of the operand preparation of the plane GEMMs (planes_gemm.h; kernels: planes_split_kernels.h): an f32
// matrix is split ONCE, in a pass of its own, into 16-bit planes laid out for the GEMM kernel's LDS-DMA stages.
//
//   np = 3: three bf16 planes, no scale.
//   np = 2: two f16 planes of the matrix scaled by a power of two s taken from its Frobenius norm -- from a norm pass over the matrix, or
//           from an upper bound a producer left (PlanesSplitArgs::fro2_bound, planes_scale_bound).  A matrix of at most 4 M elements
//           ("small") forms its scale inside the split launch; the small weight matrices of a step go as one grouped pair of launches.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>

#include "common.h"
#include "gemm_f32.h"
#include "planes_gemm.h"
#include "planes_split_kernels.h"

namespace tdnnf {

size_t planes_bytes(int np, long long rows_total, long long k_blocks) { return (size_t)(k_blocks * np * rows_total * 32); }
size_t planes_sumsq_ws_bytes() { return sizeof(double) * kSumsqBlocks; }

// rows and base 16-byte aligned: the float4 norm pass and the split's float4 reads
static bool rows_aligned16(const MatView &x) { return (reinterpret_cast<uintptr_t>(x.data) & 15) == 0 && x.stride % 4 == 0; }
// a small matrix gets as many norm-pass blocks as it has 16 K-element pieces, and its split forms the scale itself: two launches, not three
static bool planes_small(const MatView &x) { return (long long)x.rows * x.cols <= (4LL << 20); }
static int sumsq_blocks(int rows, int cols, bool small) {
  return small ? (int)std::max<long long>(1, std::min<long long>(kSumsqBlocks, ((long long)rows * cols + 16383) / 16384)) : kSumsqBlocks;
}
// the norm pass of x over nb blocks into ws[0 .. nb)
static void launch_sumsq(const MatView &x, int nb, void *ws, hipStream_t s) {
  if (rows_aligned16(x)) hipLaunchKernelGGL(planes_sumsq4_kernel, dim3(nb), dim3(256), 0, s, x, (double *)ws);
  else hipLaunchKernelGGL(planes_sumsq_kernel, dim3(nb), dim3(256), 0, s, x, (double *)ws);
}

hipError_t planes_check_bound(MatView x, const float *rec, void *sumsq_ws, hipStream_t s) {
  launch_sumsq(x, kSumsqBlocks, sumsq_ws, s);
  hipLaunchKernelGGL(planes_check_bound_kernel, dim3(1), dim3(256), 0, s, (const double *)sumsq_ws, kSumsqBlocks, rec);
  return hipGetLastError();
}
void planes_bound_counts(long long *checks, long long *violations) {
  unsigned c = 0, v = 0;
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(&c, HIP_SYMBOL(g_bound_checks), sizeof(c));
  (void)hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_bound_violations), sizeof(v));
  if (checks) *checks = c;
  if (violations) *violations = v;
}

hipError_t planes_pad(int np, void *P, long long k_blocks, long long R, int lead, long long rows, hipStream_t s) {
  if (!P || R <= rows) return hipSuccess;
  hipLaunchKernelGGL(planes_pad_kernel, dim3(grid_for(k_blocks * np * (R - rows) * 2, 256)), dim3(256), 0, s, P, k_blocks * np, R, lead, rows);
  return hipGetLastError();
}

hipError_t planes_scale_bound(const double *fro2_bound, int blocks, double numel, float mul, float add_coef, const float *add_rec, float *rec, hipStream_t s) {
  hipLaunchKernelGGL(planes_scale_kernel, dim3(1), dim3(256), 0, s, fro2_bound, blocks, numel, rec, mul, add_coef, add_rec);
  return hipGetLastError();
}

hipError_t planes_split(const PlanesSplitArgs &a, hipStream_t s) {
  const MatView &x = a.x;
  if (x.rows <= 0 || x.cols <= 0 || (!a.P && !a.PT)) return hipSuccess;
  if (a.np != 2 && a.np != 3) return hipErrorInvalidValue;
  ProfHbmRange prof(7, (double)x.rows * x.cols * (4.0 + 2.0 * a.np * ((a.P ? 1 : 0) + (a.PT ? 1 : 0))), s);  // the matrix read once, each layout written once
  const double numel = (double)x.rows * x.cols;
  const double *sq_partial = nullptr;
  int sq_nb = 0;
  hipError_t e = hipSuccess;
  if (a.np == 2) {
    if (!a.scale || !a.sumsq_ws) return hipErrorInvalidValue;
    if (a.fro2_bound && a.fro2_blocks > 0) {  // the producer's finalize launch left a bound: no pass over the matrix
      e = planes_scale_bound(a.fro2_bound, a.fro2_blocks, numel, a.fro_mul, a.add_coef, a.add_rec, a.scale, s);
      if (e == hipSuccess && options().planes_check_bound) e = planes_check_bound(x, a.scale, a.sumsq_ws, s);
    } else {
      const bool small = planes_small(x);
      sq_nb = sumsq_blocks(x.rows, x.cols, small);
      launch_sumsq(x, sq_nb, a.sumsq_ws, s);
      if (small) sq_partial = (const double *)a.sumsq_ws;
      else e = planes_scale_bound((const double *)a.sumsq_ws, sq_nb, numel, 1.0f, 0.0f, nullptr, a.scale, s);
    }
  }
  if (e == hipSuccess && !a.pads_done) e = planes_pad(a.np, a.P, planes_kblocks(x.cols), a.R, a.lead, x.rows, s);
  if (e == hipSuccess && !a.pads_done) e = planes_pad(a.np, a.PT, planes_t_kblocks(x.rows), a.Rt, 0, x.cols, s);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)((x.rows + 63) / 64), (unsigned)((x.cols + 63) / 64));
  const int vec_ok = rows_aligned16(x) ? 1 : 0;
  if (a.np == 2)
    hipLaunchKernelGGL(planes_split_kernel<2>, grid, dim3(256), 0, s, x.data, (long long)x.stride, x.rows, x.cols, (const float *)a.scale, a.lead, a.R, a.P, a.Rt, a.PT, vec_ok,
                       sq_partial, sq_nb, a.scale, a.col_coef, a.col_coef_period);
  else
    hipLaunchKernelGGL(planes_split_kernel<3>, grid, dim3(256), 0, s, x.data, (long long)x.stride, x.rows, x.cols, (const float *)nullptr, a.lead, a.R, a.P, a.Rt, a.PT, vec_ok,
                       (const double *)nullptr, 0, (float *)nullptr, a.col_coef, a.col_coef_period);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------ the grouped split
struct PlanesSplitGroup {
  std::vector<PlanesSplitItem> items;
  std::vector<int> sq_first, sp_first;
  PlanesSplitItem *d_items = nullptr;
  int *d_sq_first = nullptr, *d_sp_first = nullptr;
  double *d_partial = nullptr;
  int cap = 0, cap_partial = 0;
};
void planes_split_group_destroy(PlanesSplitGroup *g) {
  if (!g) return;
  for (void *p : {(void *)g->d_items, (void *)g->d_sq_first, (void *)g->d_sp_first, (void *)g->d_partial})
    if (p) hipFree(p);
  delete g;
}
bool planes_split_group_ok(const PlanesSplitArgs &a) {
  const MatView &x = a.x;
  return a.np == 2 && x.rows > 0 && x.cols > 0 && (a.P || a.PT) && a.scale && !(a.fro2_bound && a.fro2_blocks > 0) && a.pads_done && planes_small(x) &&
         rows_aligned16(x);
}
hipError_t planes_split_group(const std::vector<PlanesSplitArgs> &v, PlanesSplitGroup **cache, hipStream_t s) {
  if (v.empty()) return hipSuccess;
  if (!*cache) *cache = new PlanesSplitGroup();
  PlanesSplitGroup &g = **cache;
  std::vector<PlanesSplitItem> items(v.size());
  std::vector<int> sqf(v.size() + 1, 0), spf(v.size() + 1, 0);
  double bytes = 0;
  for (size_t i = 0; i < v.size(); i++) {
    const PlanesSplitArgs &a = v[i];
    if (!planes_split_group_ok(a)) return hipErrorInvalidValue;
    PlanesSplitItem it;
    memset(&it, 0, sizeof(it));
    it.X = a.x.data; it.ld = a.x.stride; it.rows = a.x.rows; it.cols = a.x.cols; it.lead = a.lead; it.R = a.R; it.Rt = a.Rt; it.P = a.P; it.PT = a.PT;
    it.scale = a.scale; it.col_coef = a.col_coef; it.col_coef_period = a.col_coef_period; it.vec_ok = 1;
    it.sq_nb = sumsq_blocks(a.x.rows, a.x.cols, true);
    it.sq_first = sqf[i];
    it.sp_gx = (a.x.rows + 63) / 64;
    it.sp_first = spf[i];
    sqf[i + 1] = sqf[i] + it.sq_nb;
    spf[i + 1] = spf[i] + it.sp_gx * ((a.x.cols + 63) / 64);
    items[i] = it;
    bytes += (double)a.x.rows * a.x.cols * (4.0 + 4.0 * ((a.P ? 1 : 0) + (a.PT ? 1 : 0)));
  }
  const bool same = g.items.size() == items.size() && memcmp(g.items.data(), items.data(), sizeof(PlanesSplitItem) * items.size()) == 0;
  if (!same) {
    if (g.cap < (int)items.size()) {
      for (void *p : {(void *)g.d_items, (void *)g.d_sq_first, (void *)g.d_sp_first})
        if (p) hipFree(p);
      hipError_t e = hipMalloc((void **)&g.d_items, sizeof(PlanesSplitItem) * items.size());
      if (e == hipSuccess) e = hipMalloc((void **)&g.d_sq_first, sizeof(int) * (items.size() + 1));
      if (e == hipSuccess) e = hipMalloc((void **)&g.d_sp_first, sizeof(int) * (items.size() + 1));
      if (e != hipSuccess) return e;
      g.cap = (int)items.size();
    }
    if (g.cap_partial < sqf.back()) {
      if (g.d_partial) hipFree(g.d_partial);
      hipError_t e = hipMalloc((void **)&g.d_partial, sizeof(double) * sqf.back());
      if (e != hipSuccess) return e;
      g.cap_partial = sqf.back();
    }
    g.items = items; g.sq_first = sqf; g.sp_first = spf;
    hipError_t e = hipMemcpyAsync(g.d_items, g.items.data(), sizeof(PlanesSplitItem) * items.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(g.d_sq_first, g.sq_first.data(), sizeof(int) * sqf.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(g.d_sp_first, g.sp_first.data(), sizeof(int) * spf.size(), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
  }
  ProfHbmRange prof(7, bytes, s);
  hipLaunchKernelGGL(planes_sumsq4_group_kernel, dim3(sqf.back()), dim3(256), 0, s, g.d_items, g.d_sq_first, (int)items.size(), g.d_partial);
  hipLaunchKernelGGL(planes_split_group_kernel, dim3(spf.back()), dim3(256), 0, s, g.d_items, g.d_sp_first, (int)items.size(), (const double *)g.d_partial);
  return hipGetLastError();
}

}  // namespace tdnnf
