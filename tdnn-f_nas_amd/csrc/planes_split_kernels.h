// planes_split_kernels.h -- the kernels that prepare a plane GEMM's operands (host side: planes_split.hip): the norm pass, the scale
// record, the split into P16 planes (one matrix or a group of small ones), the zero rows around a matrix, and the check of a norm bound.
//
//   P16 planes of an R x C matrix:  e16 P[kb][plane][row][16],  kb = c / 16 (K blocks of 16), row 0..R-1
//   (R = lead + rows + tail: zero rows in front and behind, so that row-shifted tap views and tile overhang read zeros);
//   a row record is 32 bytes, its two 16-byte halves (k 0..7 | k 8..15) swapped when bit 3 of the row index is set, which makes
//   the 16-byte fragment reads of 16 consecutive rows fall on 16 different 16-byte columns of the 256-byte LDS bank row.
//   The same pass writes the planes of the TRANSPOSE (k = row index) for the products that reduce over rows (weight gradients).
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"
#include "planes_dev.h"

namespace tdnnf {
namespace {

// ------------------------------------------------------------------------------------------------------ the norm pass
constexpr int kSumsqBlocks = 1024;
// what every norm kernel ends with: partial[b] = the block's sum of its 256 threads' `acc` (fixed order: deterministic)
__device__ __forceinline__ void planes_sumsq_block_tail(double acc, double *partial, unsigned b) {
  __shared__ double red[4];
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[b] = (red[0] + red[1]) + (red[2] + red[3]);
}
// partial[b] = sum of squares of the elements block b walks (fixed assignment: deterministic)
__global__ __launch_bounds__(256) void planes_sumsq_kernel(MatView x, double *partial) {
  const long long total = (long long)x.rows * x.cols;
  double acc = 0;
  float run = 0.f;
  int cnt = 0;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int r = (int)(e / x.cols), c = (int)(e % x.cols);
    const float v = x.data[(long long)r * x.stride + c];
    run += v * v;
    if (++cnt == 64) {  // short float runs, double across them
      acc += run;
      run = 0.f;
      cnt = 0;
    }
  }
  acc += run;
  planes_sumsq_block_tail(acc, partial, blockIdx.x);
}
// the same with 16-byte reads (rows and base 16-byte aligned): a thread owns float4 columns, a row's last few columns one by one.
// This thread's share of block b's walk when nb blocks share the matrix.
__device__ __forceinline__ double planes_sumsq4_walk(const float *X, long long ld, int rows, int cols, long long b, long long nb) {
  const int c4 = (cols + 3) >> 2;
  const long long total = (long long)rows * c4;
  double acc = 0;
  float run = 0.f;
  int cnt = 0;
  for (long long e = b * 256LL + threadIdx.x; e < total; e += nb * 256) {
    const int r = (int)(e / c4), c = (int)(e % c4);
    const float *src = X + (long long)r * ld + 4 * c;
    if (4 * c + 3 < cols) {
      const float4 v = *reinterpret_cast<const float4 *>(src);
      run += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
    } else {
      for (int j = 0; 4 * c + j < cols; j++) run += src[j] * src[j];
    }
    if (++cnt == 16) {
      acc += run;
      run = 0.f;
      cnt = 0;
    }
  }
  return acc + run;
}
__global__ __launch_bounds__(256) void planes_sumsq4_kernel(MatView x, double *partial) {
  planes_sumsq_block_tail(planes_sumsq4_walk(x.data, x.stride, x.rows, x.cols, blockIdx.x, gridDim.x), partial, blockIdx.x);
}

// ------------------------------------------------------------------------------------------------------ the scale record
// red[0] = sum of partial[0 .. nb), by the 256 threads of a block through red[256] (fixed order: every block that sums the same partials
// gets the same number); every thread may read it on return
__device__ __forceinline__ void planes_block_sum256(const double *partial, int nb, double *red) {
  double a = 0;
  for (int i = threadIdx.x; i < nb; i += 256) a += partial[i];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
}
// scale[0] = s = 2^e, the largest power of two with s ||X||_F <= 65504 (every |x| <= ||X||_F: nothing overflows) and s rms(X) <= 64;
// scale[1] = 1 / s; scale[2] = the norm (or the upper bound it was taken from).  An all-zero matrix gets s = 1; a NaN / Inf norm gives a
// NaN scale (the product is then NaN, as in f32).  With `mul` / `add_rec`: sqrt(sum) is only part of a bound, mul sqrt(sum) + add_coef add_rec[2].
// (all 256 threads of a block; every block that calls it with the same partials gets the same s: fixed summation order)
__device__ __forceinline__ float planes_scale_of(const double *partial, int nb, double numel, float mul, float add_coef, const float *add_rec, double *red,
                                                 double *fro_out) {
  planes_block_sum256(partial, nb, red);
  const double sum = red[0];
  const double fro = (double)mul * sqrt(sum) + (add_rec ? (double)add_coef * (double)add_rec[2] : 0.0);
  float s = 1.0f;
  if (fro != fro || fro > 1.0e150) {
    s = __int_as_float(0x7fc00000);
  } else if (fro > 0) {
    const double rms = fro / sqrt(numel);
    int e = (int)floor(log2(65504.0 / fro));
    const int e2 = (int)floor(log2(64.0 / rms));
    if (e2 < e) e = e2;
    if (e > 120) e = 120;
    if (e < -120) e = -120;
    s = ldexpf(1.0f, e);
  }
  *fro_out = fro;
  __syncthreads();  // (red is reused by the caller)
  return s;
}
__device__ __forceinline__ void planes_write_scale_record(float *rec, float s, double fro) {
  rec[0] = s;
  rec[1] = 1.0f / s;
  rec[2] = (float)(fro * 1.000001);  // (rounded up: the record may feed the bound of a matrix this one is added into)
}
__global__ void planes_scale_kernel(const double *partial, int nb, double numel, float *scale, float mul, float add_coef, const float *add_rec) {
  __shared__ double red[256];
  double fro;
  const float s = planes_scale_of(partial, nb, numel, mul, add_coef, add_rec, red, &fro);
  if (threadIdx.x != 0) return;
  planes_write_scale_record(scale, s, fro);
}

// ------------------------------------------------------------------------------------------------------ the split pass
// X (rows x cols, ld) -> P16 planes (k = column; `lead` zero rows in front) and / or the planes of the transpose (k = row).
// A block: a 64 x 64 tile; thread t reads 16 consecutive floats of row t / 4 (one row record of P), the transposed records go
// through LDS (thread t then owns column t % 64, rows 16 (t / 64) ..+15).
// sq_partial != null (small matrices): the scale is formed here from the norm pass's partials -- by every block, identically -- and
// block (0, 0) writes the record; saves the launch of planes_scale_kernel in front of every small split
template <int NP>
__device__ __forceinline__ void planes_split_block(const float *X, long long ld, int rows, int cols, const float *scale, int lead, long long R, void *Pv,
                                                   long long Rt, void *PTv, int vec_ok, const double *sq_partial, int sq_nb, float *scale_out,
                                                   const float *col_coef, int col_coef_period, int bx, int by) {
  typedef typename Plane<NP>::E E;
  __shared__ __attribute__((aligned(16))) E tile[NP][64][64 + 2];
  E *P = reinterpret_cast<E *>(Pv), *PT = reinterpret_cast<E *>(PTv);
  const int t = threadIdx.x, lr = t >> 2, cq = t & 3;
  const int r = bx * 64 + lr, c0 = by * 64 + cq * 16;
  float s = scale ? scale[0] : 1.0f;
  if (sq_partial) {
    double fro;
    s = planes_scale_of(sq_partial, sq_nb, (double)rows * cols, 1.0f, 0.0f, nullptr, reinterpret_cast<double *>(&tile[0][0][0]), &fro);
    if (bx == 0 && by == 0 && t == 0) planes_write_scale_record(scale_out, s, fro);
  }
  float v[16];
#pragma unroll
  for (int j = 0; j < 16; j++) v[j] = 0.f;
  if (r < rows && c0 < cols) {
    const float *src = X + (long long)r * ld + c0;
    if (vec_ok && c0 + 15 < cols) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const float4 f = *reinterpret_cast<const float4 *>(src + 4 * q);
        v[4 * q] = f.x; v[4 * q + 1] = f.y; v[4 * q + 2] = f.z; v[4 * q + 3] = f.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 16; j++)
        if (c0 + j < cols) v[j] = src[j];
    }
  }
  if (col_coef) {  // tap coefficients folded into the planes
#pragma unroll
    for (int j = 0; j < 16; j++)
      if (c0 + j < cols) v[j] *= col_coef[(c0 + j) / col_coef_period];
  }
  E pl[NP][16];
#pragma unroll
  for (int j = 0; j < 16; j++) {
    E e[NP];
    Plane<NP>::split(v[j] * s, e);
#pragma unroll
    for (int p = 0; p < NP; p++) pl[p][j] = e[p];
  }
  const int nkb = (cols + 15) / 16, kb = c0 >> 4;
  if (P && r < rows && kb < nkb) {
    const long long ra = (long long)lead + r;
    const int sw = (int)((ra >> 3) & 1);
#pragma unroll
    for (int p = 0; p < NP; p++) {
      E *dst = P + (((long long)kb * NP + p) * R + ra) * 16;
      *reinterpret_cast<uint4 *>(dst + (0 ^ sw) * 8) = *reinterpret_cast<const uint4 *>(&pl[p][0]);
      *reinterpret_cast<uint4 *>(dst + (1 ^ sw) * 8) = *reinterpret_cast<const uint4 *>(&pl[p][8]);
    }
  }
  if (!PT) return;
#pragma unroll
  for (int p = 0; p < NP; p++)
#pragma unroll
    for (int j = 0; j < 16; j++) tile[p][lr][cq * 16 + j] = pl[p][j];
  __syncthreads();
  const int c = by * 64 + (t & 63), kq = t >> 6;
  if (c >= cols) return;  // (rows of PT beyond `cols` are zeroed by the pad kernel)
  const long long kbt = (long long)bx * 4 + kq;
  const int sw = (c >> 3) & 1;
#pragma unroll
  for (int p = 0; p < NP; p++) {
    E rec[16];
#pragma unroll
    for (int j = 0; j < 16; j++) rec[j] = tile[p][kq * 16 + j][t & 63];
    E *dst = PT + ((kbt * NP + p) * Rt + c) * 16;
    *reinterpret_cast<uint4 *>(dst + (0 ^ sw) * 8) = *reinterpret_cast<const uint4 *>(&rec[0]);
    *reinterpret_cast<uint4 *>(dst + (1 ^ sw) * 8) = *reinterpret_cast<const uint4 *>(&rec[8]);
  }
}

template <int NP>
__global__ __launch_bounds__(256) void planes_split_kernel(const float *X, long long ld, int rows, int cols, const float *scale, int lead, long long R, void *Pv,
                                                           long long Rt, void *PTv, int vec_ok, const double *sq_partial, int sq_nb, float *scale_out,
                                                           const float *col_coef, int col_coef_period) {
  planes_split_block<NP>(X, ld, rows, cols, scale, lead, R, Pv, Rt, PTv, vec_ok, sq_partial, sq_nb, scale_out, col_coef, col_coef_period, (int)blockIdx.x,
                         (int)blockIdx.y);
}
// Grouped form for many SMALL matrices (a net's weight matrices at the start of a step: 36 x (norm pass + split) launches, strictly serial on
// the caller's stream, nothing else in flight): matrix i owns the blocks [first[i], first[i + 1]) of each of the two launches.
struct PlanesSplitItem {
  const float *X;
  long long ld, R, Rt;
  int rows, cols, lead, vec_ok;
  void *P, *PT;
  float *scale;
  const float *col_coef;
  int col_coef_period;
  int sq_first, sq_nb;  // its norm-pass blocks / partials: [sq_first, sq_first + sq_nb)
  int sp_first, sp_gx;  // its split blocks: sp_first + by * sp_gx + bx
};
__device__ __forceinline__ int planes_item_of(const int *first, int n, int b) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (b >= first[mid]) lo = mid;
    else hi = mid;
  }
  return lo;
}
// (planes_sumsq4_kernel's walk with the item's sq_nb blocks: the partials, hence the scale, are those of a split of its own)
__global__ __launch_bounds__(256) void planes_sumsq4_group_kernel(const PlanesSplitItem *items, const int *first, int n, double *partial) {
  const PlanesSplitItem it = items[planes_item_of(first, n, (int)blockIdx.x)];
  planes_sumsq_block_tail(planes_sumsq4_walk(it.X, it.ld, it.rows, it.cols, (int)blockIdx.x - it.sq_first, it.sq_nb), partial, blockIdx.x);
}
__global__ __launch_bounds__(256) void planes_split_group_kernel(const PlanesSplitItem *items, const int *first, int n, const double *partial) {
  const PlanesSplitItem it = items[planes_item_of(first, n, (int)blockIdx.x)];
  const int b = (int)blockIdx.x - it.sp_first;
  planes_split_block<2>(it.X, it.ld, it.rows, it.cols, it.scale, it.lead, it.R, it.P, it.Rt, it.PT, it.vec_ok, partial + it.sq_first, it.sq_nb, it.scale, it.col_coef,
                        it.col_coef_period, b % it.sp_gx, b / it.sp_gx);
}

// zero the rows [0, lead) and [lead + rows, R) of every (kb, plane) chunk (32-byte records of 2-byte elements, whatever the type)
__global__ __launch_bounds__(256) void planes_pad_kernel(void *Pv, long long nchunks, long long R, int lead, long long rows) {
  unsigned short *P = reinterpret_cast<unsigned short *>(Pv);
  const long long pad = R - rows;  // per chunk
  const long long total = nchunks * pad * 2;  // 16-byte pieces
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const long long chunk = e / (pad * 2), w = e % (pad * 2);
    long long row = w / 2;
    if (row >= lead) row += rows;
    *reinterpret_cast<uint4 *>(P + (chunk * R + row) * 16 + (w & 1) * 8) = make_uint4(0, 0, 0, 0);
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------------ the bound check
// (device variables: whoever reads them with hipMemcpyFromSymbol must be in the translation unit that includes this header --
// planes_split.hip's planes_bound_counts())
__device__ unsigned g_bound_checks = 0, g_bound_violations = 0;
__global__ void planes_check_bound_kernel(const double *partial, int nb, const float *rec) {
  __shared__ double red[256];
  planes_block_sum256(partial, nb, red);
  if (threadIdx.x != 0) return;
  atomicAdd(&g_bound_checks, 1u);
  if (!(sqrt(red[0]) <= (double)rec[2])) atomicAdd(&g_bound_violations, 1u);
}

}  // namespace tdnnf
