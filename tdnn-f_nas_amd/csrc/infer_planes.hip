// infer_planes.hip -- the f16x3 forward pass of the whole-utterance inference (tdnnf_infer_create_arith with gemm_precision 3; the
// entries: infer.hip).  The one schedule (infer_forward.hip), the same f32 activations (the bypass and the BatchNorm pass of a strided
// layer read them); every GEMM runs from f16 planes (planes_gemm.h, np 2), behind a split of its input:
//   weights      the matrices of the chosen head's path, split at the top of every compute into planes this object owns (the model is read
//                at every compute, as in f32); every tap's column block sits at its own 16-aligned K block, so a bottleneck that is no
//                multiple of 16 needs no other kernel (such a matrix is first copied with its tap blocks padded: infer_pad_taps_kernel).
//   activations  two plane buffers, alternating: a GEMM reads the planes of the previous GEMM's output and its own output is split into
//                the other buffer.  The GEMM leaves the sums of squares of what it stored (PlanesGemmArgs::colstats), from which the split
//                takes its scale (planes_scale_bound) without a pass over the matrix; the spliced input and the output of a strided
//                layer's BatchNorm pass, which no plane GEMM stored, get a norm pass.  Every split writes the zero rows of ITS geometry
//                (lead, tail) again, because the buffers hold another shape at every layer and another batch size in a compute's last
//                batch: no row of an earlier, larger matrix can be read through a tap or a tile's overhang.
//   strided rows the .affine of a layer whose input runs at a finer rate than its output reads every rho-th row of the (rho-ordered)
//                .linear output: the rows of phase p = tap offset % rho are a matrix with row stride rho, which is split into a plane
//                region of its own; a tap then reads contiguous rows of its phase's region.  All phases share one scale (one norm bound).
// The epilogue is planes_gemm_kernel's POST form (bias, ReLU, BatchNorm scale / offset, bypass, row map), launched by planes_gemm_post().
// A GEMM whose operands do not fit these rules runs on the f32 kernel (gemm_post) and is counted (tdnnf_infer_gemm_counts): never silently.
#include <string.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "gemm_f32.h"
#include "infer_forward.h"
#include "infer_planes_kernels.h"
#include "infer_state.h"
#include "net_model.h"
#include "planes_gemm.h"
#include "planes_gemm_kernels.h"
#include "prof.h"

using namespace tdnnf;

namespace tdnnf {

// ------------------------------------------------------------------------------------------------------ the GEMM launch
namespace {

template <int WM, int WN, int TM, int TN>
hipError_t launch_post(const PlanesGemmArgs &a, hipStream_t s) {
  typedef PlanesTile<2, WM, WN, TM, TN> Tile;
  static bool attr_done = false;
  if (!attr_done) {
    hipError_t e = hipFuncSetAttribute((const void *)planes_gemm_kernel<2, WM, WN, TM, TN, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, Tile::LDS_BYTES);
    if (e != hipSuccess) return e;
    attr_done = true;
  }
  const int ntm = (a.M + Tile::BM - 1) / Tile::BM, ntn = (a.N + Tile::BN - 1) / Tile::BN;
  hipLaunchKernelGGL((planes_gemm_kernel<2, WM, WN, TM, TN, false, true>), dim3(ntm * ntn), dim3(Tile::NT), (size_t)Tile::LDS_BYTES, s, a, ntm, ntn);
  return hipGetLastError();
}

}  // namespace

hipError_t planes_gemm_post(const PlanesGemmArgs &a, hipStream_t s) {
  if (a.M <= 0 || a.N <= 0 || a.nseg <= 0) return hipSuccess;
  if (a.np != 2 || a.a_rows_as_k || a.ntap > 1 || a.ksplit > 1 || a.init_mode == 0 || a.skip_coef || (a.col_scale == nullptr) != (a.col_offset == nullptr))
    return hipErrorInvalidValue;
  // planes_gemm()'s tiles (planes_gemm.hip launch_tile)
  const int bn = planes_gemm_tile_cols(a.N);
  if (bn == 160) return launch_post<8, 1, 1, 5>(a, s);
  if (bn == 128) return launch_post<4, 2, 2, 2>(a, s);
  if (planes_gemm_launch_tile_rows(a) == 128) return launch_post<2, 2, 2, 4>(a, s);
  return launch_post<4, 2, 2, 4>(a, s);
}

// ------------------------------------------------------------------------------------------------------ the object's planes
struct WPlanes {  // one weight matrix: Do x (K taps of Di columns), leading dimension ldw
  int comp, Do, K, Di, kbt;  // kbt: K blocks per tap
  float *pad;                // K > 1 and Di % 16 != 0: the copy with padded tap blocks (Do x K kbt 16), else null
  void *P;
  long long R;
  float *rec;  // [s, 1 / s, norm]
};

struct InferPlanes {
  char *arena = nullptr;
  std::vector<WPlanes> w;  // 0 lda, 1 tdnn1, 2 + 2 l / 3 + 2 l layer l's .linear / .affine, then prefinal-l and the head's affine, linear, output
  void *X[2];              // activation planes
  float *rec[2];           // their scale records
  float *colstats;         // of the last plane GEMM
  double *bound;           // kInferBoundBlocks partial sums of a norm bound
  void *ws;                // planes_split's norm-pass scratch
  PlanesSplitGroup *group = nullptr;
};

namespace {

inline long long round16(long long v) { return (v + 15) / 16 * 16; }

// How the planes of an activation lie in a plane buffer for ONE consumer (the taps of its GEMM): phase regions of Rp rows each
// (a region: `lead` zero rows, the phase's rows, zero rows up to Rp), R rows per (K block, plane) chunk in all.
struct AGeo {
  int rho, nph, phase[16], ph_of_tap[16], ntap, lead, kb;
  long long shift[16], rows_p, Rp, R;
  // what a buffer must hold for this geometry AND every smaller batch's: planes_rows_padded() adds 8 rows to some row counts, so a smaller
  // batch's R may exceed a larger one's by up to 7
  size_t bytes() const { return planes_bytes(2, R + 16, planes_slot_kblocks(16 * kb)); }
};
bool a_geometry(long long rows, int cols, const tdnnf_tdnn_indexes &ix, AGeo *g) {
  memset(g, 0, sizeof(*g));
  g->rho = ix.row_stride;
  g->ntap = ix.num_offsets;
  if (g->rho < 1 || g->ntap < 1 || g->ntap > 16 || rows % g->rho != 0) return false;
  long long max_shift = 0;
  for (int i = 0; i < g->ntap; i++) {
    const int off = ix.row_offsets[i];
    if (off < 0) return false;
    const int ph = off % g->rho;
    int pi = 0;
    while (pi < g->nph && g->phase[pi] != ph) pi++;
    if (pi == g->nph) g->phase[g->nph++] = ph;
    g->ph_of_tap[i] = pi;
    g->shift[i] = off / g->rho;
    max_shift = std::max(max_shift, g->shift[i]);
  }
  g->lead = (int)round16(max_shift);  // (the taps shift forward: the lead rows are never read, the tail covers shift + tile overhang)
  g->rows_p = rows / g->rho;
  g->kb = (int)planes_kblocks(cols);
  if (g->nph == 1) {
    g->Rp = g->R = planes_slot_rows(g->rows_p, g->lead);
  } else {
    g->Rp = round16(2LL * g->lead + g->rows_p + 256);
    g->R = planes_rows_padded(g->nph * g->Rp);
  }
  return g->R < (1LL << 31);
}

void layout(tdnnf_infer *q, InferPlanes *ip, Arena &A) {
  const tdnnf_net *n = q->model;
  const tdnnf_net_config &c = n->cfg;
  const int B = q->max_chunks, Hd = c.hidden_dim, S = c.prefinal_small_dim, P = c.num_pdfs, lda_dim = 3 * c.feat_dim + c.ivector_dim;
  const auto &H = n->head[q->which];
  ip->w.clear();
  auto add_w = [&](int comp, int Do, int K, int Di) {
    WPlanes w;
    memset(&w, 0, sizeof(w));
    w.comp = comp; w.Do = Do; w.K = K; w.Di = Di;
    w.kbt = (int)planes_kblocks(Di);
    w.R = planes_slot_t_rows(Do);
    if (K > 1 && Di % 16 != 0) w.pad = A.take<float>((size_t)Do * K * w.kbt * 16);
    w.P = A.take<char>(planes_bytes(2, w.R, planes_slot_kblocks(16 * K * w.kbt)));
    w.rec = A.take<float>(4);
    ip->w.push_back(w);
  };
  // (the order of FwdGemm's roles)
  add_w(n->c_lda, lda_dim, 1, lda_dim);
  add_w(n->tdnn1.comp, Hd, 1, lda_dim);
  size_t xbytes = 0;
  long long rows_max = 0;
  int n_max = std::max(std::max(lda_dim, Hd), S);
  AGeo g;
  auto use = [&](long long rows, int cols, const tdnnf_tdnn_indexes &ix) {
    rows_max = std::max(rows_max, rows);
    if (a_geometry(rows, cols, ix, &g)) xbytes = std::max(xbytes, g.bytes());
  };
  const tdnnf_tdnn_indexes ix1 = one_tap();
  use((long long)q->g_lda.n * B, lda_dim, ix1);
  for (const FwdLayer &Ly : infer_buffers(q, B).layers) {  // (the largest batch)
    const Tdnn &lin = Ly.lin, &aff = Ly.aff;
    add_w(lin.comp, lin.Do, lin.K, lin.Di);
    add_w(aff.comp, aff.Do, aff.K, aff.Di);
    use(lin.rows_in, Hd, lin.ix);
    use(lin.rows_out, lin.Do, aff.ix);
    rows_max = std::max(rows_max, (long long)aff.rows_out);
    n_max = std::max(n_max, lin.Do);
  }
  add_w(n->c_prefinal_l, S, 1, Hd);
  add_w(H.c_affine, Hd, 1, S);
  add_w(H.c_linear, S, 1, Hd);
  add_w(H.c_output, P, 1, S);
  use((long long)q->Tout * B, Hd, ix1);
  use((long long)q->Tout * B, S, ix1);
  for (int i = 0; i < 2; i++) {
    ip->X[i] = A.take<char>(xbytes);
    ip->rec[i] = A.take<float>(4);
  }
  ip->colstats = A.take<float>((size_t)2 * ((rows_max + 127) / 128) * n_max);  // a partial row of sums and one of sums of squares per row tile (>= 128 rows)
  ip->bound = A.take<double>(kInferBoundBlocks);
  ip->ws = A.take<char>(planes_sumsq_ws_bytes());
}

// ------------------------------------------------------------------------------------------------------ one batch
struct Fwd {
  tdnnf_infer *q;
  InferPlanes *ip;
  hipStream_t s;
  int xb = 0;           // the buffer that holds the planes of the last split matrix
  bool have = false;    // ... for the consumer described by geo
  AGeo geo;
  const float *have_of = nullptr;  // the matrix they were split from
  int stat_tiles = 0, stat_n = 0;  // > 0: colstats holds the sums of squares of the last stored matrix (stat_tiles row tiles x stat_n columns)
  long long pg = 0, fg = 0;
};

// the planes of x for the GEMM whose taps are ix, into the buffer the last GEMM did not read
int split_for(Fwd &f, const tdnnf_mat &x, const tdnnf_tdnn_indexes &ix) {
  InferPlanes *ip = f.ip;
  const int tiles = f.stat_tiles, sn = f.stat_n;
  f.stat_tiles = f.stat_n = 0;
  f.have = false;
  AGeo g;
  if (!a_geometry(x.rows, x.cols, ix, &g)) return TDNNF_OK;  // (the consumer then runs in f32, counted)
  const int xb = f.xb ^ 1;
  bool bound = false;
  if (tiles > 0 && sn == x.cols) {  // the producer's sums of squares: colstats[(tiles + tile) * N + n]
    hipLaunchKernelGGL(infer_stats_bound_kernel, dim3(kInferBoundBlocks), dim3(256), 0, f.s, ip->colstats + (long long)tiles * sn, (long long)tiles * sn, ip->bound);
    TDNNF_LAUNCH_CHECK();
    bound = true;
  } else if (g.nph > 1) {  // phases must share their scale: one norm for all of them
    hipLaunchKernelGGL(infer_sumsq_kernel, dim3(kInferBoundBlocks), dim3(256), 0, f.s, view(&x), ip->bound);
    TDNNF_LAUNCH_CHECK();
    bound = true;
  }
  if (g.nph > 1) TDNNF_HIP(hipMemsetAsync(ip->X[xb], 0, planes_bytes(2, g.R, g.kb), f.s));  // every region's zero rows
  for (int pi = 0; pi < g.nph; pi++) {
    PlanesSplitArgs a;
    a.np = 2;
    a.x = MatView{x.data + (long long)g.phase[pi] * x.stride, (int)g.rows_p, x.cols, x.stride * g.rho};
    a.P = ip->X[xb];
    a.lead = (int)(pi * g.Rp) + g.lead;
    a.R = g.R;
    a.PT = nullptr;
    a.Rt = 0;
    a.scale = ip->rec[xb];
    a.sumsq_ws = ip->ws;
    if (bound) {
      a.fro2_bound = ip->bound;
      a.fro2_blocks = kInferBoundBlocks;
      a.fro_mul = 1.0001f;  // (the partial sums were rounded to f32 on their way)
    }
    a.pads_done = g.nph > 1;
    TDNNF_HIP(planes_split(a, f.s));
  }
  f.xb = xb;
  f.geo = g;
  f.have = true;
  f.have_of = x.data;
  return TDNNF_OK;
}

// out = epilogue(in (x) W[wi]) over the taps ix, from the planes split_for(in, ix) left; in f32 where there are none
int gemm(Fwd &f, int wi, const tdnnf_tdnn_indexes &ix, const tdnnf_mat &in, int relu, const float *coef, const tdnnf_mat *add, float add_scale,
         const int *row_map, const tdnnf_mat &out, bool stats) {
  const tdnnf_net *n = f.q->model;
  const WPlanes &w = f.ip->w[wi];
  const float *W = net_W(n, w.comp), *bias = net_bias(n, w.comp);
  const AGeo &g = f.geo;
  bool ok = f.have && f.have_of == in.data && g.ntap == w.K && ix.num_offsets == w.K && ix.row_stride == g.rho && g.kb == w.kbt && in.cols == w.Di && w.K <= 32;
  for (int i = 0; ok && i < w.K; i++) ok = g.shift[i] + out.rows <= g.rows_p;  // every row a tap reads is a row of its phase
  f.stat_tiles = f.stat_n = 0;
  if (!ok) {
    f.fg++;
    return gemm_post(ix, in, W, w.K * w.Di, w.Do, w.Di, bias, relu, coef, add, add_scale, row_map, out, f.s);
  }
  PlanesGemmArgs a;
  memset(&a, 0, sizeof(a));
  a.np = 2;
  a.A = f.ip->X[f.xb];
  a.RA = g.R;
  a.B = w.P;
  a.RB = w.R;
  a.scale_a = f.ip->rec[f.xb];
  a.scale_b = w.rec;
  a.C = out.data;
  a.ldc = out.stride;
  a.M = out.rows;
  a.N = w.Do;
  a.bias = bias;
  a.init_mode = bias ? 1 : 2;
  a.relu = relu;
  a.nseg = w.K;
  for (int i = 0; i < w.K; i++) {
    a.seg[i].a_row = g.ph_of_tap[i] * g.Rp + g.lead + g.shift[i];
    a.seg[i].b_row = 0;
    a.seg[i].a_kb0 = 0;
    a.seg[i].b_kb0 = i * w.kbt;
    a.seg[i].nkb = w.kbt;
  }
  if (coef) {  // [mean | variance | scale | offset]
    a.col_scale = coef + 2 * w.Do;
    a.col_offset = coef + 3 * w.Do;
  }
  if (add) {
    a.add = add->data;
    a.ldadd = add->stride;
    a.add_scale = add_scale;
    a.add_lo = 0;
    a.add_hi = a.M;
  }
  a.row_map = row_map;
  if (stats) {
    const int bm = planes_gemm_launch_tile_rows(a);
    a.colstats = f.ip->colstats;
    a.colstats_stride = (a.M + bm - 1) / bm;
  }
  {
    const double mk = (double)a.M * w.K * w.Di, nk = (double)a.N * w.K * w.Di, mn = (double)a.M * a.N;
    ProfGemmRange prof(planes_gemm_tile_cols(a.N) == 160 ? 1 : 0, 2.0 * mk * a.N, 4.0 * (mk + nk + mn), f.s);  // (the classes of rows_gemm)
    TDNNF_HIP(planes_gemm_post(a, f.s));
  }
  if (stats) {
    f.stat_tiles = a.colstats_stride;
    f.stat_n = a.N;
  }
  f.pg++;
  return TDNNF_OK;
}

// the FwdGemm of this pass: the planes of the GEMM's input, then the GEMM (role = the index of its weight planes)
int split_and_gemm(void *ctx, hipStream_t, int role, int comp, const tdnnf_tdnn_indexes &ix, const tdnnf_mat &in, int relu, const float *coef, const tdnnf_mat *add,
                   float add_scale, const int *row_map, const tdnnf_mat &out, bool wants_stats) {
  Fwd &f = *static_cast<Fwd *>(ctx);
  CK(split_for(f, in, ix));
  return gemm(f, role, ix, in, relu, coef, add, add_scale, row_map, out, wants_stats);
}

}  // namespace

// ------------------------------------------------------------------------------------------------------ create / begin / forward
int infer_planes_create(tdnnf_infer *q) {
  InferPlanes *ip = new InferPlanes();
  Arena sizing;
  layout(q, ip, sizing);
  const size_t bytes = sizing.off + 1024;
  if (hipMalloc((void **)&ip->arena, bytes) != hipSuccess) {
    (void)hipGetLastError();
    set_error("infer_create_arith: cannot allocate %zu bytes of planes", bytes);
    delete ip;
    return TDNNF_EHIP;
  }
  Arena real;
  real.base = ip->arena;
  layout(q, ip, real);
  q->planes = ip;
  // the zero rows (and K-block padding) around every weight matrix, once: each compute splits the same shapes into the same places
  TDNNF_HIP(hipMemset(ip->arena, 0, bytes));
  return TDNNF_OK;
}

void infer_planes_destroy(InferPlanes *ip) {
  if (!ip) return;
  planes_split_group_destroy(ip->group);
  hipFree(ip->arena);
  delete ip;
}

int infer_planes_begin(tdnnf_infer *q, hipStream_t s) {
  InferPlanes *ip = q->planes;
  const tdnnf_net *n = q->model;
  std::vector<PlanesSplitArgs> grouped;
  for (const WPlanes &w : ip->w) {
    const float *W = net_W(n, w.comp);
    PlanesSplitArgs a;
    a.np = 2;
    if (w.pad) {
      const int Dp = w.kbt * 16;
      hipLaunchKernelGGL(infer_pad_taps_kernel, dim3(grid_for((long long)w.Do * w.K * Dp, 256)), dim3(256), 0, s, W, w.K * w.Di, w.Do, w.K, w.Di, Dp, w.pad);
      TDNNF_LAUNCH_CHECK();
      a.x = MatView{w.pad, w.Do, w.K * Dp, w.K * Dp};
    } else {
      a.x = MatView{const_cast<float *>(W), w.Do, w.K * w.Di, w.K * w.Di};
    }
    a.P = w.P;
    a.lead = 0;
    a.R = w.R;
    a.PT = nullptr;
    a.Rt = 0;
    a.scale = w.rec;
    a.sumsq_ws = ip->ws;
    a.pads_done = true;
    if (planes_split_group_ok(a)) grouped.push_back(a);
    else TDNNF_HIP(planes_split(a, s));
  }
  TDNNF_HIP(planes_split_group(grouped, &ip->group, s));
  return TDNNF_OK;
}

int infer_planes_forward(tdnnf_infer *q, int B, tdnnf_mat *out, hipStream_t s, FwdCounts *counts) {
  Fwd f;
  f.q = q;
  f.ip = q->planes;
  f.s = s;
  CK(infer_forward(q->model, q->head.coef, q->which, B, infer_buffers(q, B), out, split_and_gemm, &f, s, counts));
  q->plane_gemms += f.pg;
  q->f32_gemms += f.fg;
  return TDNNF_OK;
}

}  // namespace tdnnf
