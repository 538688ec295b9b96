// abi_planes.hip -- C-ABI of the pre-split plane GEMMs (include/tdnnf_hip.h): the operand split (planes_split.hip), the GEMM and its
// epilogue form (planes_gemm.hip), the sizes a caller allocates by, and the counters the tests read.
#include <string.h>

#include "common.h"
#include "planes_gemm.h"

using namespace tdnnf;

extern "C" {

size_t tdnnf_planes_bytes(int num_planes, long long rows_total, long long k_blocks) {
  if ((num_planes != 2 && num_planes != 3) || rows_total <= 0 || k_blocks <= 0) return 0;
  return planes_bytes(num_planes, rows_total, k_blocks);
}
size_t tdnnf_planes_split_workspace_bytes(void) { return planes_sumsq_ws_bytes(); }
// option planes_check_bound: how many bound-derived scales were checked against the measured norm, and how many bounds were too small
// (synchronises the device)
void tdnnf_planes_bound_checks(long long *checks, long long *violations) { planes_bound_counts(checks, violations); }
void tdnnf_planes_routed(long long *rows_gemms, long long *weight_gradients) {
  if (rows_gemms) *rows_gemms = g_planes_routed_rows;
  if (weight_gradients) *weight_gradients = g_planes_routed_wgrad;
}

int tdnnf_planes_split(int num_planes, const tdnnf_mat *x, int lead_rows, long long rows_total, void *planes, long long t_rows_total, void *planes_t,
                       float *scale_dev, void *workspace_dev, tdnnf_stream stream) {
  TDNNF_REQUIRE((num_planes == 2 || num_planes == 3) && mat_ok(x) && x->cols > 0 && lead_rows >= 0 && (planes || planes_t), "planes_split: bad arguments (2 or 3 planes)");
  TDNNF_REQUIRE(!planes || rows_total >= (long long)lead_rows + x->rows, "planes_split: rows_total must cover lead + rows");
  TDNNF_REQUIRE(!planes_t || t_rows_total >= x->cols, "planes_split: t_rows_total must cover the matrix's columns");
  TDNNF_REQUIRE(((reinterpret_cast<uintptr_t>(planes) | reinterpret_cast<uintptr_t>(planes_t)) & 15) == 0, "planes_split: the plane buffers must be 16-byte aligned");
  TDNNF_REQUIRE(num_planes == 3 || (scale_dev && workspace_dev), "planes_split: two f16 planes need the scale output and the workspace");
  PlanesSplitArgs a;
  a.np = num_planes; a.x = view(x); a.P = planes; a.lead = lead_rows; a.R = rows_total; a.PT = planes_t; a.Rt = t_rows_total; a.scale = scale_dev; a.sumsq_ws = workspace_dev;
  TDNNF_HIP(planes_split(a, (hipStream_t)stream));
  return TDNNF_OK;
}

static int planes_gemm_abi(int num_planes, const void *a_planes, long long a_rows_total, const float *a_scale_dev, const void *b_planes, long long b_rows_total,
                           const float *b_scale_dev, int num_segments, const long long *a_row, const long long *b_row, const int *a_first_col, const int *b_first_col,
                           const int *seg_cols, const float *bias, int init_mode, int relu, const tdnnf_mat *add, float add_scale, int add_first_row, float *colstats,
                           int *colstats_rows, tdnnf_mat *c, tdnnf_stream stream) {
  TDNNF_REQUIRE((num_planes == 2 || num_planes == 3) && a_planes && b_planes && mat_ok(c) && num_segments >= 1 && num_segments <= 16 && a_row && a_first_col &&
                    b_first_col && seg_cols,
                "planes_gemm: bad arguments (2 or 3 planes, 1..16 segments)");
  TDNNF_REQUIRE(init_mode >= 0 && init_mode <= 2 && (init_mode != 1 || bias), "planes_gemm: init_mode 0 (+=), 1 (bias), 2 (=)");
  TDNNF_REQUIRE(!add || (mat_ok(add) && add->cols == c->cols && add_first_row >= 0), "planes_gemm: the addend must have the output's columns");
  PlanesGemmArgs a;
  memset(&a, 0, sizeof(a));
  a.np = num_planes;
  a.A = a_planes; a.RA = a_rows_total; a.B = b_planes; a.RB = b_rows_total; a.scale_a = a_scale_dev; a.scale_b = b_scale_dev;
  a.C = c->data; a.ldc = c->stride; a.M = c->rows; a.N = c->cols;
  a.bias = bias; a.init_mode = init_mode; a.relu = relu; a.nseg = num_segments;
  if (add) {
    a.add = add->data; a.ldadd = add->stride; a.add_scale = add_scale; a.add_lo = add_first_row; a.add_hi = add_first_row + add->rows;
  }
  const int BM = planes_gemm_tile_rows(c->cols), BN = planes_gemm_tile_cols(c->cols);
  for (int i = 0; i < num_segments; i++) {
    const long long br = b_row ? b_row[i] : 0;
    TDNNF_REQUIRE(a_first_col[i] % 16 == 0 && b_first_col[i] % 16 == 0 && seg_cols[i] > 0 && a_row[i] >= 0 && br >= 0, "planes_gemm: segment %d: columns must start on a multiple of 16", i);
    TDNNF_REQUIRE(a_row[i] + (long long)((c->rows + BM - 1) / BM) * BM <= a_rows_total,
                  "planes_gemm: segment %d reads rows %lld..%lld of an A plane buffer of %lld rows (tail rows must cover the %d-row tile)", i, a_row[i],
                  a_row[i] + (long long)((c->rows + BM - 1) / BM) * BM, a_rows_total, BM);
    TDNNF_REQUIRE(br + (long long)((c->cols + BN - 1) / BN) * BN <= b_rows_total, "planes_gemm: segment %d: the B plane buffer needs %lld rows (output columns padded to the %d-column tile)", i,
                  br + (long long)((c->cols + BN - 1) / BN) * BN, BN);
    a.seg[i].a_row = a_row[i];
    a.seg[i].b_row = br;
    a.seg[i].a_kb0 = a_first_col[i] / 16;
    a.seg[i].b_kb0 = b_first_col[i] / 16;
    a.seg[i].nkb = (seg_cols[i] + 15) / 16;
  }
  if (colstats) {  // one partial row per row tile of THIS launch (the tile height depends on the shape), sums first, sums of squares behind them
    TDNNF_REQUIRE(colstats_rows, "planes_gemm: colstats_rows must be given with colstats");
    const int tile_rows = planes_gemm_launch_tile_rows(a);
    a.colstats = colstats;
    a.colstats_stride = (c->rows + tile_rows - 1) / tile_rows;
    *colstats_rows = (int)a.colstats_stride;
  }
  TDNNF_HIP(planes_gemm(a, (hipStream_t)stream));
  return TDNNF_OK;
}

int tdnnf_planes_gemm(int num_planes, const void *a_planes, long long a_rows_total, const float *a_scale_dev, const void *b_planes, long long b_rows_total,
                      const float *b_scale_dev, int num_segments, const long long *a_row, const long long *b_row, const int *a_first_col, const int *b_first_col,
                      const int *seg_cols, const float *bias, int init_mode, int relu, tdnnf_mat *c, tdnnf_stream stream) {
  return planes_gemm_abi(num_planes, a_planes, a_rows_total, a_scale_dev, b_planes, b_rows_total, b_scale_dev, num_segments, a_row, b_row, a_first_col, b_first_col, seg_cols,
                         bias, init_mode, relu, nullptr, 0.f, 0, nullptr, nullptr, c, stream);
}

int tdnnf_planes_gemm_epilogue(int num_planes, const void *a_planes, long long a_rows_total, const float *a_scale_dev, const void *b_planes, long long b_rows_total,
                               const float *b_scale_dev, int num_segments, const long long *a_row, const long long *b_row, const int *a_first_col,
                               const int *b_first_col, const int *seg_cols, const float *bias, int init_mode, int relu, const tdnnf_mat *add, float add_scale,
                               int add_first_row, float *colstats, int *colstats_rows, tdnnf_mat *c, tdnnf_stream stream) {
  return planes_gemm_abi(num_planes, a_planes, a_rows_total, a_scale_dev, b_planes, b_rows_total, b_scale_dev, num_segments, a_row, b_row, a_first_col, b_first_col, seg_cols,
                         bias, init_mode, relu, add, add_scale, add_first_row, colstats, colstats_rows, c, stream);
}

}  // extern "C"
