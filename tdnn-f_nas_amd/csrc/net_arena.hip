// net_arena.hip -- the one device allocation behind a tdnnf_net: every activation, statistics block, derivative scratch, plane slot,
// natural-gradient buffer and workspace, carved in a fixed order by a sequence of named parts.  net_create.hip runs net_layout_arena
// twice: with a null base to size the allocation, then over it.  The parts also latch the options that decide which buffers exist
// (wg_lag, wg_on, planes_np, ng_grouped, early_on, early_group), so that the step reads what the layout was made for.  A net made by
// tdnnf_net_create_shared carves its own statistics blocks too (unused: it adopts the primary's), so there is one layout.
#include <string>

#include "common.h"
#include "fused.h"
#include "gemm_f32.h"
#include "gemm_ring.h"
#include "net_model.h"
#include "ng.h"

namespace tdnnf {
namespace {

// row counts the parts share
struct Rows {
  int N0, No;        // rows of the lda / tdnn1 grid and of the output grid
  int max_rows;      // the tallest hidden_dim-wide matrix of the trunk
  int max_lin_rows;  // the tallest bottleneck matrix
  int big_rows() const { return std::max(max_rows, std::max(N0, No)); }
};
Rows rows_of(const tdnnf_net *n) {
  Rows r{N_of(n->g_lda, n->B), n->Tout * n->B, 0, 0};
  r.max_rows = r.N0;
  for (auto &L : n->layers) {
    r.max_rows = std::max(r.max_rows, std::max(N_of(L.gout, n->B), N_of(L.gin, n->B)));
    r.max_lin_rows = std::max(r.max_lin_rows, N_of(L.lin.out, n->B));
  }
  return r;
}
// the two bottleneck-wide derivative matrices and their lag-3 seconds: wide enough for the heads' prefinal_small_dim and for any bottleneck
float *small_mat(const tdnnf_net *n, Arena &A, const Rows &r) {
  return A.mat(std::max(r.max_lin_rows, r.No), std::max(n->cfg.prefinal_small_dim, 512));
}
size_t bsum_floats(const CompDesc &cd) { return ((size_t)cd.rows + 15) & ~(size_t)15; }  // a component's raw bias gradient, 64-byte blocks

void take_activations(tdnnf_net *n, Arena &A, const Rows &r) {
  const tdnnf_net_config &c = n->cfg;
  const int B = n->B, Hd = c.hidden_dim, S = c.prefinal_small_dim, P = c.num_pdfs;
  const int lda_dim = 3 * c.feat_dim + c.ivector_dim;
  n->lda_in = A.mat(r.N0, lda_dim);
  n->lda_out = A.mat(r.N0, lda_dim);
  n->t1_relu = A.mat(r.N0, Hd);
  n->t1_bn = A.mat(r.N0, Hd);
  n->t1_bn_memo = A.take<float>(bn_memo_floats(Hd));
  n->t1_bn_stats = A.take<double>(bn_stats_doubles(Hd));
  n->t1_relu_stats = A.take<double>(relu_stats_doubles(Hd));
  for (auto &L : n->layers) {
    const int nl = N_of(L.lin.out, B), no = N_of(L.gout, B);
    L.lin_out = A.mat(nl, L.bn);
    L.lin_perm = L.perm ? A.mat(nl, L.bn) : nullptr;
    L.arch_p = L.arch_mask = L.lin_masked = nullptr;
    if (L.c_arch >= 0) {
      L.arch_p = A.take<float>(8);
      L.arch_mask = A.take<float>(L.bn + 4);
      L.lin_masked = A.mat(nl, L.bn);
    }
    L.relu_out = A.mat(no, Hd);
    L.noop_out = A.mat(no, Hd);
    L.bn_memo = A.take<float>(bn_memo_floats(Hd));
    L.lin.memo = L.lin.darts ? A.take<float>(2 * TDNNF_MAX_OFFSETS) : nullptr;
    L.aff.memo = L.aff.darts ? A.take<float>(2 * TDNNF_MAX_OFFSETS) : nullptr;
    L.lin.active = L.lin.darts ? A.take<int>(TDNNF_MAX_OFFSETS + 1) : nullptr;
    L.aff.active = L.aff.darts ? A.take<int>(TDNNF_MAX_OFFSETS + 1) : nullptr;
    L.bn_stats = A.take<double>(bn_stats_doubles(Hd));
    L.relu_stats = A.take<double>(relu_stats_doubles(Hd));
  }
  n->prefinal_l_out = A.mat(r.No, S);
  for (int h = 0; h < 2; h++) {
    auto &H = n->head[h];
    H.aff_relu = A.mat(r.No, Hd);
    H.bn1_out = A.mat(r.No, Hd);
    H.lin_out = A.mat(r.No, S);
    H.bn2_out = A.mat(r.No, S);
    H.y = A.mat(r.No, P);
    H.bn1_memo = A.take<float>(bn_memo_floats(Hd));
    H.bn2_memo = A.take<float>(bn_memo_floats(S));
    H.bn1_stats = A.take<double>(bn_stats_doubles(Hd));
    H.bn2_stats = A.take<double>(bn_stats_doubles(S));
    H.relu_stats = A.take<double>(relu_stats_doubles(Hd));
  }
  n->xent_logsoftmax = A.mat(r.No, P);
}

// derivative matrices, the step's gradient and what else the backward pass scratches in
void take_backward_scratch(tdnnf_net *n, Arena &A, const Rows &r) {
  const tdnnf_net_config &c = n->cfg;
  const int B = n->B, Hd = c.hidden_dim, S = c.prefinal_small_dim, P = c.num_pdfs;
  n->d_y = A.mat(r.No, P);
  n->d_xent = A.mat(r.No, P);
  n->dA = A.mat(r.max_rows, Hd);
  n->dB = A.mat(r.max_rows, Hd);
  n->dC = A.mat(r.max_rows, Hd);
  n->d_small = small_mat(n, A, r);
  n->d_small2 = small_mat(n, A, r);
  // weight gradients three components behind the caller's stream (wg_lag 3, net.h): a second buffer for the derivative the affine's
  // gradient reads, two more for what the linear's reads -- layers alternate between them
  n->wg_lag = options().wgrad_lag == 1 ? 1 : 3;
  n->wg_on = options().wgrad_stream >= 0 ? options().wgrad_stream != 0 : r.max_rows <= 32768;
  const bool lag3 = n->wg_on && n->wg_lag == 3;
  n->dC2 = lag3 ? A.mat(r.max_rows, Hd) : nullptr;
  n->dS[0] = lag3 ? small_mat(n, A, r) : nullptr;
  n->dS[1] = lag3 ? small_mat(n, A, r) : nullptr;
  size_t tg = 0;
  for (auto &L : n->layers)
    if (L.lin.darts) tg = std::max(tg, (size_t)L.bn * L.lin.K * Hd);
  n->tapgrad = tg ? A.take<float>(tg) : nullptr;
  n->tapdots = A.take<double>(TDNNF_TAP_DOTS_DOUBLES(TDNNF_MAX_OFFSETS));
  n->bn_sync.buf = A.take<double>(5 * (size_t)std::max(std::max(Hd, S), 1) + 8);  // (the ReLU backward sweep stages five column sums)
  n->dropout_masks = (c.use_dropout && !c.cv_update) ? A.take<float>((size_t)(c.num_layers + 1) * B * Hd) : nullptr;
  n->gtmp = A.take<float>((size_t)n->num_params + 16);
  // transposed copy of every weight matrix for the split-bf16 backward-data GEMMs (k-contiguous B operand).  (Measured for exact
  // f32 too, twice: no gain -- docs/experiments.md.)
  n->paramsT = (c.gemm_precision == 1 || c.gemm_precision == 2) ? A.take<float>((size_t)n->num_params + 16) : nullptr;
}

// pre-split plane operands (net.h): a slot per GEMM operand matrix, keyed by its base pointer, and the weight matrices' planes
void take_planes(tdnnf_net *n, Arena &A, const Rows &r) {
  const tdnnf_net_config &c = n->cfg;
  const int B = n->B, Hd = c.hidden_dim, S = c.prefinal_small_dim, P = c.num_pdfs, lda_dim = 3 * c.feat_dim + c.ivector_dim;
  n->planes_np = c.gemm_precision == 3 ? 2 : (c.gemm_precision == 2 && options().planes ? 3 : 0);
  n->plane_slots.clear();
  n->pw.assign(n->comps.size(), PlanesOperand());
  n->pw_scale.assign(n->comps.size(), nullptr);
  n->planes_ws = nullptr;
  n->fro_buf = nullptr;
  if (!n->planes_np) return;
  const int np = n->planes_np;
  int lead_cap = 0;  // the largest row shift of a backward-data view (taps of rho == 1 layers)
  for (auto &L : n->layers) lead_cap = std::max(lead_cap, std::max(max_off(L.lin), max_off(L.aff)));
  auto slot = [&](const float *key, int rows, int cols, bool with_lead) {
    const long long R = planes_slot_rows(rows, with_lead ? (lead_cap + 15) & ~15 : 0);
    const long long Rt = planes_slot_t_rows(cols);
    tdnnf_net::PlaneSlot ps;
    ps.bytesP = planes_bytes(np, R, planes_slot_kblocks(cols));
    ps.bytesPT = planes_bytes(np, Rt, planes_t_kblocks(rows));
    ps.P = A.take<char>(ps.bytesP + 64);
    ps.PT = A.take<char>(ps.bytesPT + 64);
    ps.scale = A.take<float>(4);
    if (A.base) n->plane_slots[key] = ps;
  };
  const int small_rows = std::max(r.max_lin_rows, r.No), small_cols = std::max(S, 512);
  slot(n->lda_out, r.N0, lda_dim, false);
  slot(n->t1_bn, r.N0, Hd, false);
  for (auto &L : n->layers) {
    slot(L.noop_out, N_of(L.gout, B), Hd, false);
    slot(L.lin_out, N_of(L.lin.out, B), L.bn, false);
    if (L.c_arch >= 0) slot(L.lin_masked, N_of(L.lin.out, B), L.bn, false);  // (bottleneck supernet: the affine reads the masked blocks)
  }
  slot(n->prefinal_l_out, r.No, S, false);
  for (int h = 0; h < 2; h++) {
    slot(n->head[h].bn1_out, r.No, Hd, false);
    slot(n->head[h].bn2_out, r.No, S, false);
  }
  slot(n->d_y, r.No, P, false);
  slot(n->d_xent, r.No, P, false);
  slot(n->dA, r.big_rows(), Hd, true);
  slot(n->dB, r.big_rows(), Hd, true);
  slot(n->dC, r.big_rows(), Hd, true);
  slot(n->d_small, small_rows, small_cols, true);
  slot(n->d_small2, small_rows, small_cols, true);
  n->planes_ws = A.take<char>(planes_sumsq_ws_bytes() + 64);
  n->fro_buf = A.take<double>(finalize_grid(std::max(Hd, S)) + 8);
  // the weight matrices: row-major planes (forward: one row per output, k contiguous) and transposed planes (backward-data)
  for (size_t i = 0; i < n->comps.size(); i++) {
    const CompDesc &cd = n->comps[i];
    if (cd.plain || cd.rows < 2 || (int)i == n->c_lda) continue;
    PlanesOperand &o = n->pw[i];
    o.rows = cd.rows; o.cols = cd.cols; o.ld = cd.cols; o.np = np; o.lead = 0;
    o.R = planes_slot_t_rows(cd.rows);  // (a weight matrix's rows are the tile columns of its forward GEMM)
    o.Rt = planes_slot_t_rows(cd.cols);
    o.P = A.take<char>(planes_bytes(np, o.R, planes_kblocks(cd.cols)) + 64);
    o.PT = A.take<char>(planes_bytes(np, o.Rt, planes_t_kblocks(cd.rows)) + 64);
    n->pw_scale[i] = A.take<float>(4);
    o.scale = n->pw_scale[i];
  }
}

// the transpose of the largest constrained matrix with more rows than columns; returns the workspace ConstrainOrthonormal needs on it
size_t take_ortho_transpose(tdnnf_net *n, Arena &A) {
  size_t tall = 0, tall_ws = 0;
  for (auto &cd : n->comps)
    if (cd.orthonormal != 0.f && cd.rows > cd.cols) {
      tall = std::max(tall, (size_t)cd.rows * cd.cols);
      tall_ws = std::max(tall_ws, tdnnf_constrain_orthonormal_workspace_bytes(cd.cols, cd.rows));
    }
  n->orthoT = tall ? A.take<float>(tall + 16) : nullptr;
  return tall_ws;
}

// per-component buffers of the N-sized passes and the side chain's scratch; returns the shared-workspace bytes the statistics passes need
size_t take_natural_gradient(tdnnf_net *n, Arena &A, const Rows &r) {
  n->s3_scratch = nullptr;
  n->s3_scratch_bytes = 0;
  n->ng_grouped = options().ng_grouped != 0;  // 0: the per-object side chain for every component
  n->ngc.assign(n->comps.size(), tdnnf_net::NgComp());
  if (!n->cfg.use_natural_gradient) return 0;
  size_t ng_ws = 0, mtmp = 0;
  for (const WeightComp &w : weight_comps(n)) {
    const CompDesc &cd = n->comps[w.comp];
    if (!cd.updatable || cd.plain) continue;  // (sized whatever the learning-rate factor is: an edit may unfreeze a component)
    const int Dx = cd.cols + (cd.has_bias ? 1 : 0), ldT = (Dx + 3) & ~3, rows = w.rows_out;
    int rank_in, rank_out;
    ng_ranks(cd, &rank_in, &rank_out);
    const int Rpi = (rank_in + 3) & ~3, Rpo = (rank_out + 3) & ~3;
    mtmp = std::max(mtmp, std::max((size_t)cd.rows * Rpi, (size_t)Rpo * ldT));
    ng_ws = std::max(ng_ws, std::max(ng_stats_workspace_bytes(rank_in, Dx, w.K, rows), ng_stats_workspace_bytes(rank_out, cd.rows, 1, rows)));
    auto &C = n->ngc[w.comp];
    C.N = rows;
    C.H_in = A.take<float>((size_t)rows * Rpi + 64);
    C.H_out = A.take<float>((size_t)rows * Rpo + 64);
    C.T = A.take<float>((size_t)cd.rows * ldT + 16);
    C.part_in = A.take<double>((size_t)rows_gemm_sumsq_blocks(rows) + 8);
    C.part_out = A.take<double>((size_t)rows_gemm_sumsq_blocks(rows) + 8);
  }
  // the raw bias gradients: one block for all components, zeroed once per step
  size_t tot = 0;
  for (size_t i = 0; i < n->comps.size(); i++)
    if (n->ngc[i].N > 0) tot += bsum_floats(n->comps[i]);  // (N, not the pointers: the sizing pass has none)
  n->ng_bsum_floats = tot;
  n->ng_bsum_all = A.take<float>(tot + 16);
  size_t o = 0;
  for (size_t i = 0; i < n->comps.size(); i++)
    if (n->ngc[i].N > 0) {
      n->ngc[i].bsum = n->ng_bsum_all ? n->ng_bsum_all + o : nullptr;
      o += bsum_floats(n->comps[i]);
    }
  n->ngset_ws_bytes = wgrad_workspace_bytes(80, 80, 1, r.big_rows()) + 256;
  n->ngTmp = A.take<float>(mtmp + 64);
  n->ng_side_ws = A.take<char>(n->ngset_ws_bytes);
  n->s3_scratch_bytes = 16u << 20;
  n->s3_scratch = A.take<float>(n->s3_scratch_bytes / sizeof(float));
  return ng_ws;
}

// shared workspace: wgrad slabs, column reductions, orthonormal -- the maximum over everything the caller's stream runs in it
void take_workspace(tdnnf_net *n, Arena &A, const Rows &r, size_t ng_ws, size_t tall_ws) {
  const tdnnf_net_config &c = n->cfg;
  const int Hd = c.hidden_dim, S = c.prefinal_small_dim, P = c.num_pdfs;
  size_t ws = 0;
  auto upd = [&](size_t b) { ws = std::max(ws, b); };
  for (const WeightComp &w : weight_comps(n)) {
    const CompDesc &cd = n->comps[w.comp];
    upd(wgrad_workspace_bytes(cd.rows, cd.cols / w.K, w.K, w.rows_out));
  }
  upd(colreduce_bytes(r.max_rows, Hd));
  upd(sizeof(float) * 2 * (size_t)Hd * rows_gemm_colstats_cap(r.big_rows()));  // BatchNorm partials out of the GEMM epilogue
  upd(bn_relu_bwd_workspace_bytes(r.max_rows, Hd));
  for (auto &L : n->layers) upd(tdnnf_constrain_orthonormal_workspace_bytes(L.bn, L.lin.K * Hd));
  upd(colreduce_bytes(r.No, P));
  upd(tdnnf_constrain_orthonormal_workspace_bytes(S, Hd));
  upd(tdnnf_max_change_workspace_bytes((int)n->comps.size()));
  upd(ng_ws);
  upd(tall_ws);
  if (c.bn_num_choices > 0) upd(sizeof(float) * (size_t)((r.max_lin_rows + 511) / 512 + 1) * 512);
  n->ws_bytes = ws + 256;
  n->ws = A.take<char>(n->ws_bytes);
}

// a workspace and a split-K scratch of their own for the side streams that run GEMMs beside the caller's stream
void take_side_streams(tdnnf_net *n, Arena &A) {
  // (input-side statistics ahead of the backward pass: for minibatches whose GEMMs fill the chip.  With the weight-gradient streams three
  // components behind the caller's stream the small minibatches lose by it -- 150 x 64 11.98 -> 11.25 ms, 1500 x 16 22.12 -> 21.60 on one box
  // with it off: the statistics then run with their component's gradient instead of in front of the heads' gradients.  Option ng_early_in 2 forces it.)
  // (option ng_early_in 3, weight-gradient streams on: the passes of ALL components as ONE grouped launch on s4 -- rows_gemm_group, 33 launches of
  // 26 .. 78 blocks each at 150 x 64 -- and J of a refresh step left to the component's own gradient call.  Measured 11.01 against 10.92 ms at
  // 150 x 64, 21.28 / 21.28 at 1500 x 16: fewer launches, the same work, no faster -- off.)
  n->early_on = n->cfg.use_natural_gradient && n->ng_grouped && (options().ng_early_in >= 2 || (options().ng_early_in != 0 && !n->wg_on));
  n->early_group = n->early_on && n->wg_on && options().ng_early_in == 3;
  const bool s4_used = n->wg_on || n->early_on;
  n->ws4 = s4_used ? A.take<char>(n->ws_bytes) : nullptr;
  n->s4_scratch_bytes = s4_used ? (32u << 20) : 0;
  n->s4_scratch = s4_used ? A.take<float>(n->s4_scratch_bytes / sizeof(float)) : nullptr;
  const bool two = n->wg_on && options().wgrad_stream != 1;  // (option wgrad_stream: 1 = one weight-gradient stream as rounds 2-3, 2 = two, -1 = by size, two)
  n->ws2 = two ? A.take<char>(n->ws_bytes) : nullptr;
  n->s2_scratch = two ? A.take<float>(n->s4_scratch_bytes / sizeof(float)) : nullptr;
  // (option wgrad_stream 3: a third weight-gradient stream, s5 -- beside s4 from the start of the backward pass, beside s4 and s2 once the denominator has joined)
  const bool three = two && options().wgrad_stream == 3;
  n->ws5 = three ? A.take<char>(n->ws_bytes) : nullptr;
  n->s5_scratch = three ? A.take<float>(n->s4_scratch_bytes / sizeof(float)) : nullptr;
}

}  // namespace

void net_layout_arena(tdnnf_net *n, Arena &A) {
  const Rows r = rows_of(n);
  take_activations(n, A, r);
  take_backward_scratch(n, A, r);
  take_planes(n, A, r);
  const size_t tall_ws = take_ortho_transpose(n, A);
  const size_t ng_ws = take_natural_gradient(n, A, r);
  take_workspace(n, A, r, ng_ws, tall_ws);
  take_side_streams(n, A);
}

// named activations for parity tests
void net_name_activations(tdnnf_net *n) {
  const tdnnf_net_config &c = n->cfg;
  const int B = n->B, Hd = c.hidden_dim, S = c.prefinal_small_dim, P = c.num_pdfs, lda_dim = 3 * c.feat_dim + c.ivector_dim;
  const int N0 = N_of(n->g_lda, B), No = n->Tout * B;
  auto name = [&](const std::string &s, float *p, int rows, int cols) { n->named.push_back({s, M(p, rows, cols)}); };
  name("lda", n->lda_out, N0, lda_dim);
  name("tdnn1.relu", n->t1_relu, N0, Hd);
  name("tdnn1.batchnorm", n->t1_bn, N0, Hd);
  for (int l = 0; l < c.num_layers; l++) {
    TdnnfLayer &L = n->layers[l];
    const std::string p = "tdnnf" + std::to_string(l + 2);
    name(p + ".linear", L.lin_out, L.lin.rows_out, L.bn);
    name(p + ".relu", L.relu_out, L.aff.rows_out, Hd);
    name(p + ".noop", L.noop_out, L.aff.rows_out, Hd);
  }
  if (!n->layers.empty() && !n->layers[0].perm)  // what the last backward step left: d objective / d tdnnf2.linear (debugging aid)
    name("tdnnf2.linear.deriv", n->dS[0] ? n->dS[(c.num_layers - 1) & 1] : n->d_small, n->layers[0].lin.rows_out, n->layers[0].bn);
  name("prefinal-l", n->prefinal_l_out, No, S);
  for (int h = 0; h < 2; h++) name(std::string("prefinal-") + head_name(h) + ".relu", n->head[h].aff_relu, No, Hd);
  name("output", n->head[0].y, No, P);
  name("output-xent", n->xent_logsoftmax, No, P);
  name("output.deriv", n->d_y, No, P);
}

}  // namespace tdnnf
