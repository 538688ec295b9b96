// net.hip -- the chain trainer's network for the TDNN-F graphs of the reference recipes: graph bookkeeping, arena layout,
// creation / destruction, accessors, and the optimizer step.  One minibatch of nnet3-chain-train on it (forward, chain
// objective, backward) is net_step.hip.
//
// Mirrors (UPSTREAM) NnetChainTrainer::TrainInternal; here the part behind Backprop: the shipped optimizer helpers
// ApplyL2Regularization, UpdateNnetWithMaxChange, ConstrainOrthonormal (/root/reference/src/nnet3/nnet-utils.cc:2223-2245,
// :2085-2175, :1040-1077).  Graph: /root/reference/local/chain_NAS/run_tdnn_fbk_40_iv_sp_7q.sh:160-186;
// one tdnnf-layer = steps/libs/nnet3/xconfig/composite_layers.py:135-215, prefinal-layer :1283-1331.
//
// Time bookkeeping replaces the nnet3 compiler for these graphs: every layer's output lives on a regular
// grid (t0, step, n) in t-major row order (row = k*B + b), derived backwards from the output grid
// (0, 3, T/3) exactly as the compiler's dependency analysis would (tdnnf4.linear is computed on the
// padded step-1 grid, as TdnnComponent::ReorderIndexes pads it).
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "common.h"
#include "fused.h"
#include "gemm_f32.h"
#include "gemm_ring.h"
#include "net.h"
#include "ng.h"
#include "optim_group.h"

namespace tdnnf {
namespace {

// per-component table for the update kernels
struct UpdTable {
  long long begin[129];
  float lr[128];
  float l2coef[128];
};

// out (cols x rows) = in (rows x cols)^T, both dense
__global__ void transpose_kernel(const float *in, int rows, int cols, float *out) {
  const long long total = (long long)rows * cols;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int r = (int)(e / cols), c = (int)(e % cols);
    out[(size_t)c * rows + r] = in[e];
  }
}
// ScaleBatchnormStats: every BatchNorm's [count, sum[D], sumsq[D]] *= s in one launch (block row = one component)
struct ScaleTable {
  double *p[48];
  int n[48];
};
__global__ void scale_doubles_kernel(ScaleTable tb, double s) {
  double *x = tb.p[blockIdx.y];
  const int n = tb.n[blockIdx.y];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) x[i] *= s;
}
// lda input: [feats(k+j, b), j < S ; ivector(b)]
__global__ void splice_input_kernel(MatView feats, MatView iv, int B, int S, MatView out) {
  const int C = out.cols, fd = feats.cols;
  const long long total = (long long)out.rows * C;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int r = (int)(e / C), c = (int)(e % C), k = r / B, b = r % B;
    float v;
    if (c < S * fd) v = feats.data[(size_t)((k + c / fd) * B + b) * feats.stride + c % fd];
    else v = iv.data[(size_t)b * iv.stride + (c - S * fd)];
    out.data[(size_t)r * out.stride + c] = v;
  }
}
__global__ void reorder_rows_kernel(MatView in, int B, int rho, int to_rho, MatView out) {
  const int C = in.cols;
  const long long total = (long long)in.rows * C;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += gridDim.x * 256LL) {
    const int r = (int)(e / C), c = (int)(e % C);
    const int tau = r / B, b = r % B;  // plain t-major coordinates
    const int pr = (tau / rho) * rho * B + b * rho + tau % rho;
    if (to_rho) out.data[(size_t)pr * out.stride + c] = in.data[(size_t)r * in.stride + c];
    else out.data[(size_t)r * out.stride + c] = in.data[(size_t)pr * in.stride + c];
  }
}

}  // namespace
}  // namespace tdnnf

using namespace tdnnf;

namespace {

void make_tdnn(Tdnn *t, int comp, int Di, int Do, const std::vector<int> &offs, const Grid &in, const Grid &out, int B) {
  const int K = (int)offs.size();
  t->comp = comp;
  t->Di = Di;
  t->Do = Do;
  t->K = K;
  t->darts = false;
  t->share = 0;
  t->draw0 = 0;
  t->memo = nullptr;
  t->active = nullptr;
  for (int i = 0; i < K; i++) t->offsets[i] = offs[i];
  t->in = in;
  t->out = out;
  memset(&t->ix, 0, sizeof(t->ix));
  const int rho = out.step / in.step;
  t->ix.row_stride = rho;
  t->ix.num_offsets = K;
  for (int i = 0; i < K; i++) {  // PrecomputeIndexes, nnet-tdnn-component.cc:878-903
    const int req = out.t0 + t->offsets[i];
    const int input_t = (req - in.t0) / in.step;
    t->ix.row_offsets[i] = rho * (input_t / rho) * B + input_t % rho;
  }
  t->rows_in = in.n * B;
  t->rows_out = out.n * B;
}


struct Arena {
  size_t off = 0;
  char *base = nullptr;
  template <class T>
  T *take(size_t n) {
    off = (off + 255) & ~(size_t)255;
    T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
    off += sizeof(T) * n;
    return p;
  }
  float *mat(int rows, int cols) { return take<float>((size_t)rows * ldpad(cols)); }
};

int add_comp(tdnnf_net *n, const std::string &name, int rows, int cols, int has_bias, float lr_factor, float l2, float mc,
             float ortho, int num_alpha = 0) {
  CompDesc c;
  c.num_alpha = num_alpha;
  c.name = name;
  c.begin = n->num_params;
  c.rows = rows;
  c.cols = cols;
  c.has_bias = has_bias;
  c.lr_factor = lr_factor;
  c.l2 = l2;
  c.max_change = mc;
  c.orthonormal = ortho;
  n->num_params += c.size();
  n->num_params = (n->num_params + 3) & ~3LL;  // keep every matrix 16-byte aligned
  n->comps.push_back(c);
  return (int)n->comps.size() - 1;
}

// carve (or, with base == nullptr, just size) every activation buffer
void layout_arena(tdnnf_net *n, Arena &A) {
  const tdnnf_net_config &c = n->cfg;
  const int B = n->B, Hd = c.hidden_dim, S = c.prefinal_small_dim, P = c.num_pdfs;
  const int lda_dim = 3 * c.feat_dim + c.ivector_dim;
  const int N0 = N_of(n->g_lda, B);
  n->lda_in = A.mat(N0, lda_dim);
  n->lda_out = A.mat(N0, lda_dim);
  n->t1_relu = A.mat(N0, Hd);
  n->t1_bn = A.mat(N0, Hd);
  n->t1_bn_memo = A.take<float>(5 * Hd);
  n->t1_bn_stats = A.take<double>(1 + 2 * Hd);
  n->t1_relu_stats = A.take<double>(2 + 3 * Hd);  // [count, value_sum, deriv_sum, oderiv_count, oderiv_sumsq]
  int max_rows = N0, max_lin_rows = 0;
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
    L.bn_memo = A.take<float>(5 * Hd);
    L.lin.memo = L.lin.darts ? A.take<float>(2 * TDNNF_MAX_OFFSETS) : nullptr;
    L.aff.memo = L.aff.darts ? A.take<float>(2 * TDNNF_MAX_OFFSETS) : nullptr;
    L.lin.active = L.lin.darts ? A.take<int>(TDNNF_MAX_OFFSETS + 1) : nullptr;
    L.aff.active = L.aff.darts ? A.take<int>(TDNNF_MAX_OFFSETS + 1) : nullptr;
    L.bn_stats = A.take<double>(1 + 2 * Hd);
    L.relu_stats = A.take<double>(2 + 3 * Hd);
    max_rows = std::max(max_rows, std::max(no, N_of(L.gin, B)));
    max_lin_rows = std::max(max_lin_rows, nl);
  }
  const int No = n->Tout * B;
  n->prefinal_l_out = A.mat(No, S);
  for (int h = 0; h < 2; h++) {
    auto &H = n->head[h];
    H.aff_relu = A.mat(No, Hd);
    H.bn1_out = A.mat(No, Hd);
    H.lin_out = A.mat(No, S);
    H.bn2_out = A.mat(No, S);
    H.y = A.mat(No, P);
    H.bn1_memo = A.take<float>(5 * Hd);
    H.bn2_memo = A.take<float>(5 * S);
    H.bn1_stats = A.take<double>(1 + 2 * Hd);
    H.bn2_stats = A.take<double>(1 + 2 * S);
    H.relu_stats = A.take<double>(2 + 3 * Hd);
  }
  n->xent_logsoftmax = A.mat(No, P);
  n->d_y = A.mat(No, P);
  n->d_xent = A.mat(No, P);
  n->dA = A.mat(max_rows, Hd);
  n->dB = A.mat(max_rows, Hd);
  n->dC = A.mat(max_rows, Hd);
  n->d_small = A.mat(std::max(max_lin_rows, No), std::max(S, 512));
  n->d_small2 = A.mat(std::max(max_lin_rows, No), std::max(S, 512));
  // weight gradients three components behind the caller's stream (wg_lag 3, net.h): a second buffer for the derivative the affine's
  // gradient reads, two more for what the linear's reads -- layers alternate between them
  n->wg_lag = options().wgrad_lag == 1 ? 1 : 3;
  const bool wg_size = options().wgrad_stream >= 0 ? options().wgrad_stream != 0 : std::max(max_rows, N0) <= 32768;
  const bool lag3 = wg_size && n->wg_lag == 3;
  n->dC2 = lag3 ? A.mat(max_rows, Hd) : nullptr;
  n->dS[0] = lag3 ? A.mat(std::max(max_lin_rows, No), std::max(S, 512)) : nullptr;
  n->dS[1] = lag3 ? A.mat(std::max(max_lin_rows, No), std::max(S, 512)) : nullptr;
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
  n->paramsT = (n->cfg.gemm_precision == 1 || n->cfg.gemm_precision == 2) ? A.take<float>((size_t)n->num_params + 16) : nullptr;
  // ---- pre-split plane operands (net.h): a slot per GEMM operand matrix, keyed by its base pointer
  n->planes_np = n->cfg.gemm_precision == 3 ? 2 : (n->cfg.gemm_precision == 2 && options().planes ? 3 : 0);
  n->plane_slots.clear();
  n->pw.assign(n->comps.size(), PlanesOperand());
  n->pw_scale.assign(n->comps.size(), nullptr);
  n->planes_ws = nullptr;
  n->fro_buf = nullptr;
  if (n->planes_np) {
    const int np = n->planes_np;
    int lead_cap = 0;  // the largest row shift of a backward-data view (taps of rho == 1 layers)
    for (auto &L : n->layers)
      for (const Tdnn *td : {&L.lin, &L.aff})
        for (int i = 0; i < td->K; i++) lead_cap = std::max(lead_cap, td->ix.row_offsets[i]);
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
    const int big_rows = std::max(max_rows, std::max(N0, No)), small_rows = std::max(max_lin_rows, No), small_cols = std::max(S, 512);
    slot(n->lda_out, N0, lda_dim, false);
    slot(n->t1_bn, N0, Hd, false);
    for (auto &L : n->layers) {
      slot(L.noop_out, N_of(L.gout, B), Hd, false);
      slot(L.lin_out, N_of(L.lin.out, B), L.bn, false);
      if (L.c_arch >= 0) slot(L.lin_masked, N_of(L.lin.out, B), L.bn, false);  // (bottleneck supernet: the affine reads the masked blocks)
    }
    slot(n->prefinal_l_out, No, S, false);
    for (int h = 0; h < 2; h++) {
      slot(n->head[h].bn1_out, No, Hd, false);
      slot(n->head[h].bn2_out, No, S, false);
    }
    slot(n->d_y, No, P, false);
    slot(n->d_xent, No, P, false);
    slot(n->dA, big_rows, Hd, true);
    slot(n->dB, big_rows, Hd, true);
    slot(n->dC, big_rows, Hd, true);
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
  n->s3_scratch = nullptr;
  n->s3_scratch_bytes = 0;
  n->ng_grouped = options().ng_grouped != 0;  // 0: the per-object side chain for every component
  size_t tall = 0, tall_ws = 0;
  for (auto &cd : n->comps)
    if (cd.orthonormal != 0.f && cd.rows > cd.cols) {
      tall = std::max(tall, (size_t)cd.rows * cd.cols);
      tall_ws = std::max(tall_ws, tdnnf_constrain_orthonormal_workspace_bytes(cd.cols, cd.rows));
    }
  n->orthoT = tall ? A.take<float>(tall + 16) : nullptr;
  size_t ng_ws = 0;
  n->ngc.assign(n->comps.size(), tdnnf_net::NgComp());
  if (n->cfg.use_natural_gradient) {
    size_t mtmp = 0;
    auto comp_ng = [&](int comp, int K, int rows) {  // rows = N of the component's output grid
      const CompDesc &cd = n->comps[comp];
      if (!cd.updatable || cd.plain) return;  // (sized whatever the learning-rate factor is: an edit may unfreeze a component)
      const int Dx = cd.cols + (cd.has_bias ? 1 : 0), ldT = (Dx + 3) & ~3;
      const int rank_in = std::min(20, (Dx + 1) / 2), rank_out = std::min(80, (cd.rows + 1) / 2);
      const int Rpi = (rank_in + 3) & ~3, Rpo = (rank_out + 3) & ~3;
      mtmp = std::max(mtmp, std::max((size_t)cd.rows * Rpi, (size_t)Rpo * ldT));
      ng_ws = std::max(ng_ws, std::max(ng_stats_workspace_bytes(rank_in, Dx, K, rows), ng_stats_workspace_bytes(rank_out, cd.rows, 1, rows)));
      auto &S = n->ngc[comp];
      S.N = rows;
      S.H_in = A.take<float>((size_t)rows * Rpi + 64);
      S.H_out = A.take<float>((size_t)rows * Rpo + 64);
      S.T = A.take<float>((size_t)cd.rows * ldT + 16);
      S.bsum = nullptr;  // (carved below: one block for all components, zeroed once per step)
      S.part_in = A.take<double>((size_t)rows_gemm_sumsq_blocks(rows) + 8);
      S.part_out = A.take<double>((size_t)rows_gemm_sumsq_blocks(rows) + 8);
    };
    const int No_ = n->Tout * B;
    comp_ng(n->tdnn1.comp, 1, N0);
    for (auto &L : n->layers) {
      comp_ng(L.lin.comp, L.lin.K, L.lin.rows_out);
      comp_ng(L.aff.comp, L.aff.K, L.aff.rows_out);
    }
    comp_ng(n->c_prefinal_l, 1, No_);
    for (int h = 0; h < 2; h++) {
      comp_ng(n->head[h].c_affine, 1, No_);
      comp_ng(n->head[h].c_linear, 1, No_);
      comp_ng(n->head[h].c_output, 1, No_);
    }
    {
      size_t tot = 0;
      for (size_t i = 0; i < n->comps.size(); i++)
        if (n->ngc[i].N > 0) tot += ((size_t)n->comps[i].rows + 15) & ~(size_t)15;  // (N, not the pointers: the sizing pass has none)
      n->ng_bsum_floats = tot;
      n->ng_bsum_all = A.take<float>(tot + 16);
      size_t o = 0;
      for (size_t i = 0; i < n->comps.size(); i++)
        if (n->ngc[i].N > 0) {
          n->ngc[i].bsum = n->ng_bsum_all ? n->ng_bsum_all + o : nullptr;
          o += ((size_t)n->comps[i].rows + 15) & ~(size_t)15;
        }
    }
    const size_t maxN = (size_t)std::max(std::max(max_rows, N0), No_);
    n->ngset_ws_bytes = wgrad_workspace_bytes(80, 80, 1, (int)maxN) + 256;
    n->ngTmp = A.take<float>(mtmp + 64);
    n->ng_side_ws = A.take<char>(n->ngset_ws_bytes);
    n->s3_scratch_bytes = 16u << 20;
    n->s3_scratch = A.take<float>(n->s3_scratch_bytes / sizeof(float));
  }
  // shared workspace: wgrad slabs, column reductions, orthonormal
  size_t ws = 0;
  auto upd = [&](size_t b) { ws = std::max(ws, b); };
  upd(wgrad_workspace_bytes(Hd, lda_dim, 1, N0));
  upd(colreduce_bytes(max_rows, Hd));
  upd(sizeof(float) * 2 * (size_t)Hd * rows_gemm_colstats_cap(std::max(max_rows, std::max(N0, No))));  // BatchNorm partials out of the GEMM epilogue
  upd(bn_relu_bwd_workspace_bytes(max_rows, Hd));
  for (auto &L : n->layers) {
    upd(wgrad_workspace_bytes(L.lin.Do, L.lin.Di, L.lin.K, L.lin.rows_out));
    upd(wgrad_workspace_bytes(L.aff.Do, L.aff.Di, L.aff.K, L.aff.rows_out));
    upd(tdnnf_constrain_orthonormal_workspace_bytes(L.bn, L.lin.K * Hd));
  }
  upd(wgrad_workspace_bytes(S, Hd, 1, No));
  upd(wgrad_workspace_bytes(Hd, S, 1, No));
  upd(wgrad_workspace_bytes(P, S, 1, No));
  upd(colreduce_bytes(No, P));
  upd(tdnnf_constrain_orthonormal_workspace_bytes(S, Hd));
  upd(tdnnf_max_change_workspace_bytes((int)n->comps.size()));
  upd(ng_ws);
  upd(tall_ws);
  if (n->cfg.bn_num_choices > 0) upd(sizeof(float) * (size_t)((max_lin_rows + 511) / 512 + 1) * 512);
  n->ws_bytes = ws + 256;
  n->ws = A.take<char>(n->ws_bytes);
  n->wg_on = options().wgrad_stream >= 0 ? options().wgrad_stream != 0 : std::max(max_rows, N0) <= 32768;
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

namespace tdnnf {
// the grids of every tdnnf layer for Tout output frames (stride, taps, bottleneck, gout / glin / gin, perm), derived backwards from the
// output grid; *g_lda = the first layer's input grid
int net_layer_grids(const tdnnf_net_config &c, int Tout, std::vector<TdnnfLayer> &layers, Grid *g_lda) {
  layers.resize(c.num_layers);
  Grid g{0, c.frame_subsampling, Tout};
  for (int l = c.num_layers - 1; l >= 0; l--) {
    TdnnfLayer &L = layers[l];
    L.stride = c.time_stride[l];
    L.left = c.use_layer_offsets ? c.offset_left[l] : L.stride;
    L.right = c.use_layer_offsets ? c.offset_right[l] : L.stride;
    L.bn = c.bottleneck_dim[l];
    TDNNF_REQUIRE(L.bn > 0 && L.bn <= 512 && L.left >= 0 && L.right >= 0 && L.left <= 64 && L.right <= 64,
                  "net_create: layer %d: bottleneck-dim must be in 1..512, time-stride / layer offsets in 0..64", l);
    L.gout = g;
    L.perm = false;
    Grid lin = g, in = g;
    const int Kd = c.darts_num_offsets;
    if (Kd >= 2) {
      // offset supernet: taps -(K-1)..0 / 0..K-1 at the input frame rate on every layer
      if (g.step == 1) {
        lin = Grid{g.t0, 1, g.n + Kd - 1};
      } else {
        const int rho = g.step;
        const int cnt = rho * (g.n - 1) + Kd;
        lin = Grid{g.t0, 1, ((cnt + rho - 1) / rho) * rho};  // padded to a multiple of rho (:841-843)
        L.perm = true;
      }
      in = Grid{lin.t0 - (Kd - 1), 1, lin.n + Kd - 1};
    } else if (L.left > 0 || L.right > 0) {
      // X.linear taps {-a, 0}, X.affine taps {0, b} (time-stride s: a = b = s; a derived child: any a, b >= 0).  The
      // linear runs on the coarsest regular grid that holds every frame the affine needs and whose own taps stay on the
      // input grid: step gcd(output step, a, b).  When that is finer than the output grid the affine has row_stride
      // rho > 1 and the grid is padded to a multiple of rho (nnet-tdnn-component.cc:841-843).
      const int a = L.left, b = L.right;
      auto gcd = [](int x, int y) {
        while (y) {
          const int t = x % y;
          x = y;
          y = t;
        }
        return x;
      };
      const int ls = gcd(gcd(g.step, a), b);
      if (ls == g.step) {
        lin = Grid{g.t0, g.step, g.n + b / g.step};
      } else {
        const int rho = g.step / ls, cnt = ((g.n - 1) * g.step + b) / ls + 1;
        lin = Grid{g.t0, ls, ((cnt + rho - 1) / rho) * rho};
        L.perm = true;
      }
      in = Grid{lin.t0 - a, ls, lin.n + a / ls};
    }
    L.glin = lin;
    L.gin = in;
    g = in;
  }
  *g_lda = g;
  return TDNNF_OK;
}
void net_make_tdnn(Tdnn *t, int comp, int Di, int Do, const std::vector<int> &offs, const Grid &in, const Grid &out, int B) {
  make_tdnn(t, comp, Di, Do, offs, in, out, B);
}
}  // namespace tdnnf

extern "C" {

int tdnnf_splice_input(const tdnnf_mat *feats, const tdnnf_mat *iv, int B, int S, tdnnf_mat *out, tdnnf_stream stream) {
  TDNNF_REQUIRE(mat_ok(feats) && mat_ok(iv) && mat_ok(out) && B > 0 && S > 0, "splice_input: bad arguments");
  TDNNF_REQUIRE(out->rows % B == 0 && feats->rows == (out->rows / B + S - 1) * B && iv->rows == B &&
                    out->cols == S * feats->cols + iv->cols,
                "splice_input: feats must have out_frames + num_splice - 1 time steps and out.cols = S*feat_dim + ivector_dim");
  if (out->rows == 0) return TDNNF_OK;
  hipLaunchKernelGGL(splice_input_kernel, dim3(grid_for((long long)out->rows * out->cols, 256)), dim3(256), 0, (hipStream_t)stream,
                     view(feats), view(iv), B, S, view(out));
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

int tdnnf_reorder_rows(const tdnnf_mat *in, int B, int rho, int to_rho, tdnnf_mat *out, tdnnf_stream stream) {
  TDNNF_REQUIRE(mat_ok(in) && mat_ok(out) && same_dim(in, out) && B > 0 && rho >= 1 && in->rows % (B * rho) == 0 && in->data != out->data,
                "reorder_rows: rows must be a multiple of num_seq*rho and in != out");
  if (in->rows == 0) return TDNNF_OK;
  hipLaunchKernelGGL(reorder_rows_kernel, dim3(grid_for((long long)in->rows * in->cols, 256)), dim3(256), 0, (hipStream_t)stream,
                     view(in), B, rho, to_rho, view(out));
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

static int net_create_impl(const tdnnf_net_config *cfg, const tdnnf_net *share, tdnnf_net **out);

int tdnnf_net_create(const tdnnf_net_config *cfg, tdnnf_net **out) { return net_create_impl(cfg, nullptr, out); }

int tdnnf_net_create_shared(const tdnnf_net_config *cfg, const tdnnf_net *primary, tdnnf_net **out) {
  TDNNF_REQUIRE(primary, "net_create_shared: null primary net");
  return net_create_impl(cfg, primary, out);
}

static int net_create_impl(const tdnnf_net_config *cfg, const tdnnf_net *share, tdnnf_net **out) {
  TDNNF_REQUIRE(cfg && out, "net_create: null argument");
  const tdnnf_net_config &c = *cfg;
  TDNNF_REQUIRE(c.feat_dim > 0 && c.ivector_dim > 0 && c.num_pdfs > 0 && c.hidden_dim > 0 && c.prefinal_small_dim > 0,
                "net_create: dims must be positive");
  TDNNF_REQUIRE(c.num_layers >= 1 && c.num_layers <= TDNNF_NET_MAX_LAYERS, "net_create: 1..%d tdnnf layers", TDNNF_NET_MAX_LAYERS);
  TDNNF_REQUIRE(c.darts_num_offsets == 0 || (c.darts_num_offsets >= 2 && c.darts_num_offsets <= TDNNF_MAX_OFFSETS),
                "net_create: darts_num_offsets must be 0 or 2..%d (the reference assumes K >= 2, nnet-tdnn-component.cc:232)", TDNNF_MAX_OFFSETS);
  if (c.bn_num_choices != 0) {
    TDNNF_REQUIRE(c.bn_num_choices >= 2 && c.bn_num_choices <= 8 && c.bn_mode >= 0 && c.bn_mode <= 2, "net_create: bn_num_choices must be 2..8, bn_mode 0..2");
    TDNNF_REQUIRE(c.darts_num_offsets == 0, "net_create: the bottleneck and the offset supernet cannot be combined");
    TDNNF_REQUIRE(c.bn_mode != 2 || c.bn_temp_proportion > 0, "net_create: bn_temp_proportion must be > 0");
    int sum = 0;
    for (int k = 0; k < c.bn_num_choices; k++) {
      TDNNF_REQUIRE(c.bn_choice_dims[k] > 0, "net_create: bn_choice_dims must be positive");
      sum += c.bn_choice_dims[k];
    }
    TDNNF_REQUIRE(sum <= 512, "net_create: bottleneck supernet wider than 512");
    for (int l = 0; l < c.num_layers; l++)
      TDNNF_REQUIRE(c.bottleneck_dim[l] == sum, "net_create: bottleneck_dim[%d] = %d but the choice blocks sum to %d", l, c.bottleneck_dim[l], sum);
  }
  TDNNF_REQUIRE(c.gemm_precision >= 0 && c.gemm_precision <= 3,
                "net_create: gemm_precision must be 0 (f32), 1 (split-bf16, 3 products), 2 (split-bf16, 6 products) or 3 (pre-split scaled f16 pairs, 3 products)");
  TDNNF_REQUIRE(c.darts_num_offsets == 0 || !(c.darts_flags & TDNNF_DARTS_USE_GUMBEL) || c.darts_temp_proportion > 0,
                "net_create: gumbel mode needs temp-proportion > 0");
  TDNNF_REQUIRE(c.frame_subsampling >= 1 && c.frames_per_chunk > 0 && c.frames_per_chunk % c.frame_subsampling == 0 && c.num_sequences > 0,
                "net_create: frames_per_chunk must be a positive multiple of frame_subsampling");
  tdnnf_net *n = new tdnnf_net();
  n->cfg = c;
  n->num_params = 0;
  n->params = n->grads = nullptr;
  n->arena = nullptr;
  n->B = c.num_sequences;
  n->T = c.frames_per_chunk;
  n->Tout = c.frames_per_chunk / c.frame_subsampling;
  const int B = n->B, Hd = c.hidden_dim, S = c.prefinal_small_dim, P = c.num_pdfs, lda_dim = 3 * c.feat_dim + c.ivector_dim;
  // ---- grids, derived backwards from the output grid
  CK(net_layer_grids(c, n->Tout, n->layers, &n->g_lda));
  const Grid g = n->g_lda;
  n->g_feat = Grid{g.t0 - 1, 1, g.n * g.step + 2};
  TDNNF_REQUIRE(g.step == 1, "net_create: the first tdnnf layers must run at the input frame rate");
  // ---- components, in nnet3 config order
  n->c_lda = add_comp(n, "lda", lda_dim, lda_dim, 1, 0.f, 0.f, 0.f, 0.f);
  n->comps[n->c_lda].updatable = false;
  const int c_t1 = add_comp(n, "tdnn1.affine", Hd, lda_dim, 1, 1.f, c.l2_hidden, c.max_change_hidden, 0.f);
  make_tdnn(&n->tdnn1, c_t1, lda_dim, Hd, std::vector<int>{0}, n->g_lda, n->g_lda, B);
  n->num_draws = 0;
  n->draws = nullptr;
  for (int l = 0; l < c.num_layers; l++) {
    TdnnfLayer &L = n->layers[l];
    const int Kd = c.darts_num_offsets;
    const bool darts = Kd >= 2;
    const int K = darts ? Kd : 0;  // taps of a searched component
    std::vector<int> lin_off, aff_off;
    if (darts) {
      for (int i = 0; i < K; i++) {
        lin_off.push_back(-(K - 1) + i);
        aff_off.push_back(i);
      }
    } else {  // a zero offset leaves a single tap ("time-offsets=0", composite_layers.py:145-150, generate_top_list.py:109-118)
      lin_off = L.left > 0 ? std::vector<int>{-L.left, 0} : std::vector<int>{0};
      aff_off = L.right > 0 ? std::vector<int>{0, L.right} : std::vector<int>{0};
    }
    const int Kl = (int)lin_off.size(), Ka = (int)aff_off.size();
    char nm[64];
    L.c_arch = -1;
    L.arch_draw0 = 0;
    if (c.bn_num_choices > 0) {
      // X.softmax (OnehotFunctionComponent, is-updatable=true use-natural-gradient=false) or X.alpha
      // (ConstantFunctionComponent, same flags): a C-vector, no l2, no per-component max-change
      snprintf(nm, sizeof(nm), c.bn_mode == 0 ? "tdnnf%d.softmax" : "tdnnf%d.alpha", l + 2);
      L.c_arch = add_comp(n, nm, c.bn_num_choices, 1, 0, 1.f, 0.f, 0.f, 0.f);
      n->comps[L.c_arch].plain = true;
      L.arch_draw0 = n->num_draws;
      n->num_draws += c.bn_mode == 0 ? 1 : (c.bn_mode == 2 ? c.bn_num_choices : 0);
    }
    snprintf(nm, sizeof(nm), "tdnnf%d.linear", l + 2);
    // DARTS: bias forced on (scripts/generate_config.py:25-26), K logits in front of it, and the orthonormal
    // constraint is inert because ConstrainOrthonormal does not match TdnnDARTSV3Component (nnet-utils.cc:1047-1061)
    const int cl = add_comp(n, nm, L.bn, Kl * Hd, darts ? 1 : 0, 1.f, c.l2_hidden, c.max_change_hidden, darts ? 0.f : -1.0f, darts ? K : 0);
    snprintf(nm, sizeof(nm), "tdnnf%d.affine", l + 2);
    const int ca = add_comp(n, nm, Hd, Ka * L.bn, 1, 1.f, c.l2_hidden, c.max_change_hidden, 0.f, darts ? K : 0);
    make_tdnn(&L.lin, cl, Hd, L.bn, lin_off, L.gin, L.glin, B);
    make_tdnn(&L.aff, ca, L.bn, Hd, aff_off, L.glin, L.gout, B);
    if (darts) {
      L.lin.darts = L.aff.darts = true;
      L.lin.share = K - 1;  // time_offsets_[1] < 0  (nnet-tdnn-component.cc:237-240)
      L.aff.share = 0;      // time_offsets_[1] > 0  (:232-236)
      L.lin.draw0 = n->num_draws;
      L.aff.draw0 = n->num_draws + K + 1;
      n->num_draws += 2 * (K + 1);
    }
  }
  n->dropout_draw0 = n->num_draws;
  n->dropout_proportion = 0.f;
  if (c.use_dropout && !c.cv_update) n->num_draws += (c.num_layers + 1) * B * Hd;  // one B x Hd mask per GeneralDropoutComponent
  n->c_prefinal_l = add_comp(n, "prefinal-l", S, Hd, 0, 1.f, c.l2_hidden, c.max_change_hidden, -1.0f);
  const char *hn[2] = {"chain", "xent"};
  for (int h = 0; h < 2; h++) {
    char nm[64];
    snprintf(nm, sizeof(nm), "prefinal-%s.affine", hn[h]);
    n->head[h].c_affine = add_comp(n, nm, Hd, S, 1, 1.f, c.l2_hidden, c.max_change_hidden, 0.f);
    snprintf(nm, sizeof(nm), "prefinal-%s.linear", hn[h]);
    n->head[h].c_linear = add_comp(n, nm, S, Hd, 0, 1.f, c.l2_hidden, c.max_change_hidden, -1.0f);
    // output-xent: learning-rate-factor = 0.5 / xent_regularize (run_tdnn_fbk_40_iv_sp_7q.sh:151,184)
    const float lrf = h == 1 && c.xent_regularize > 0 ? 0.5f / c.xent_regularize : 1.f;
    n->head[h].c_output = add_comp(n, h == 0 ? "output.affine" : "output-xent.affine", P, S, 1, lrf, c.l2_output,
                                   c.max_change_output, 0.f);
  }
  TDNNF_REQUIRE(n->comps.size() <= 128, "net_create: too many components");
  if (c.cv_update) {
    // cross-validation architecture update (run_TDNN_DARTSV3_fbk_stride_cvupdate.sh:128-142,
    // run_TDNNf_DARTS_mod_fbk_bottleneckCBshare_cvupdate_flopsconstraint.sh:136-139): "set-learning-rate-factor 0" on
    // everything, 1e-4 on the TdnnDARTSV3Components (theta is frozen only by that factor, the logits are compensated by
    // update-alpha's x10000), the freshly added X.alpha vectors keep factor 1.
    for (auto &cd : n->comps) cd.lr_factor = cd.plain ? 1.0f : (cd.num_alpha > 0 ? 1.0e-4f : 0.0f);
  }
  n->owns_ng = share == nullptr;
  if (share) {  // another minibatch shape of the same model: same components, the primary's preconditioners
    bool same = share->comps.size() == n->comps.size() && share->num_params == n->num_params &&
                (share->cfg.use_natural_gradient != 0) == (c.use_natural_gradient != 0) && share->cfg.cv_update == c.cv_update;
    for (size_t i = 0; same && i < n->comps.size(); i++)
      same = share->comps[i].name == n->comps[i].name && share->comps[i].rows == n->comps[i].rows && share->comps[i].cols == n->comps[i].cols &&
             share->comps[i].begin == n->comps[i].begin;
    if (!same) {
      delete n;
      TDNNF_REQUIRE(false, "net_create_shared: the configuration describes another model than the primary net's");
    }
    n->ng_in = share->ng_in;
    n->ng_out = share->ng_out;
    n->oderiv_nonzero = share->oderiv_nonzero;
  } else if (c.use_natural_gradient) {
    // one input-side and one output-side preconditioner per updatable component; configuration of
    // TdnnDARTSV3Component::InitFromConfig (nnet-tdnn-component.cc:183-210), the same defaults as
    // NaturalGradientAffineComponent / LinearComponent
    n->ng_in.assign(n->comps.size(), nullptr);
    n->ng_out.assign(n->comps.size(), nullptr);
    for (size_t i = 0; i < n->comps.size(); i++) {
      const CompDesc &cd = n->comps[i];
      if (!cd.updatable || cd.plain) continue;  // fixed lda layer; vectors updated without natural gradient
      const int spliced = cd.cols + (cd.has_bias ? 1 : 0);
      const int rank_in = std::min(20, (spliced + 1) / 2), rank_out = std::min(80, (cd.rows + 1) / 2);
      if (tdnnf_ng_create(rank_in, 4, 2000.0f, 4.0f, &n->ng_in[i]) || tdnnf_ng_create(rank_out, 4, 2000.0f, 4.0f, &n->ng_out[i])) {
        tdnnf_net_destroy(n);
        return TDNNF_EINVAL;
      }
    }
  }
  // ---- gradient buckets: whole layers, cut from the top of the flat buffer downwards (= the order backward finishes them)
  {
    const long long target = 4LL << 20;  // >= 16 MB of fp32 per collective (xGMI rings want large messages), layers kept whole
    auto first_comp_of_layer = [&](int l) { return n->layers[l].c_arch >= 0 ? n->layers[l].c_arch : n->layers[l].lin.comp; };
    long long end = n->num_params;
    tdnnf_net::GradBucket b{n->comps[n->c_prefinal_l].begin, end, -2, nullptr, nullptr};
    n->buckets.push_back(b);
    end = b.begin;
    for (int l = c.num_layers - 1; l >= 0; l--) {
      const long long begin = n->comps[first_comp_of_layer(l)].begin;
      if (end - begin >= target) {
        n->buckets.push_back(tdnnf_net::GradBucket{begin, end, l, nullptr, nullptr});
        end = begin;
      }
    }
    n->buckets.push_back(tdnnf_net::GradBucket{0, end, -1, nullptr, nullptr});
    for (auto &gb : n->buckets)
      if (hipEventCreateWithFlags(&gb.ready, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&gb.handoff, hipEventDisableTiming) != hipSuccess) {
        set_error("net_create: cannot create events");
        delete n;
        return TDNNF_EHIP;
      }
  }
  // ---- activations
  Arena sizing;
  layout_arena(n, sizing);
  n->arena_bytes = sizing.off + 1024;
  n->chain_ws = nullptr;
  n->chain_ws_bytes = 0;
  n->s2 = nullptr;
  n->wg_two = false;
  n->ev_fork = n->ev_den = n->ev_num = nullptr;
  n->s3 = nullptr;
  n->ev_s3 = nullptr;
  n->ev_fin0 = n->ev_fin = nullptr;
  n->s4 = nullptr;
  n->s5 = nullptr;
  n->ev_pg[0] = n->ev_pg[1] = n->ev_pg[2] = n->ev_pg[3] = n->ev_pg_in = nullptr;
  n->pg_count = 0;
  if (hipMalloc((void **)&n->arena, n->arena_bytes) != hipSuccess) {
    set_error("net_create: cannot allocate %zu bytes of activations", n->arena_bytes);
    delete n;
    return TDNNF_EHIP;
  }
  hipMemset(n->arena, 0, n->arena_bytes);
  Arena real;
  real.base = n->arena;
  layout_arena(n, real);
  if (share) {  // the model's BatchNorm / ReLU statistics live in the primary net
    n->t1_bn_stats = share->t1_bn_stats;
    n->t1_relu_stats = share->t1_relu_stats;
    for (size_t l = 0; l < n->layers.size(); l++) {
      n->layers[l].bn_stats = share->layers[l].bn_stats;
      n->layers[l].relu_stats = share->layers[l].relu_stats;
    }
    for (int h = 0; h < 2; h++) {
      n->head[h].bn1_stats = share->head[h].bn1_stats;
      n->head[h].bn2_stats = share->head[h].bn2_stats;
      n->head[h].relu_stats = share->head[h].relu_stats;
    }
  }
  // named activations for parity tests
  auto name = [&](const std::string &s, float *p, int rows, int cols) { n->named.push_back({s, M(p, rows, cols)}); };
  name("lda", n->lda_out, N_of(n->g_lda, B), lda_dim);
  name("tdnn1.relu", n->t1_relu, N_of(n->g_lda, B), Hd);
  name("tdnn1.batchnorm", n->t1_bn, N_of(n->g_lda, B), Hd);
  for (int l = 0; l < c.num_layers; l++) {
    TdnnfLayer &L = n->layers[l];
    const std::string p = "tdnnf" + std::to_string(l + 2);
    name(p + ".linear", L.lin_out, L.lin.rows_out, L.bn);
    name(p + ".relu", L.relu_out, L.aff.rows_out, Hd);
    name(p + ".noop", L.noop_out, L.aff.rows_out, Hd);
  }
  if (!n->layers.empty() && !n->layers[0].perm)  // what the last backward step left: d objective / d tdnnf2.linear (debugging aid)
    name("tdnnf2.linear.deriv", n->dS[0] ? n->dS[(c.num_layers - 1) & 1] : n->d_small, n->layers[0].lin.rows_out, n->layers[0].bn);
  name("prefinal-l", n->prefinal_l_out, n->Tout * B, S);
  name("prefinal-chain.relu", n->head[0].aff_relu, n->Tout * B, Hd);
  name("prefinal-xent.relu", n->head[1].aff_relu, n->Tout * B, Hd);
  name("output", n->head[0].y, n->Tout * B, P);
  name("output-xent", n->xent_logsoftmax, n->Tout * B, P);
  name("output.deriv", n->d_y, n->Tout * B, P);
  *out = n;
  return TDNNF_OK;
}

void tdnnf_net_destroy(tdnnf_net *n) {
  if (!n) return;
  if (n->s3) hipStreamSynchronize(n->s3);  // its kernels use the preconditioners' buffers
  if (n->s4) hipStreamSynchronize(n->s4);
  if (n->s5) hipStreamSynchronize(n->s5);
  if (n->s2) hipStreamSynchronize(n->s2);
  for (auto &nb : n->ng_buckets) ng_group_destroy(nb.group);
  ng_fin_destroy(n->ngfin);
  if (n->ev_ngc) hipEventDestroy(n->ev_ngc);
  if (n->owns_ng) {
    for (auto *g : n->ng_in) tdnnf_ng_destroy(g);
    for (auto *g : n->ng_out) tdnnf_ng_destroy(g);
  }
  hipFree(n->arena);
  hipFree(n->chain_ws);
  for (float *p : n->captured) hipFree(p);
  for (auto &gb : n->buckets) {
    if (gb.ready) hipEventDestroy(gb.ready);
    if (gb.handoff) hipEventDestroy(gb.handoff);
  }
  if (n->s2) hipStreamDestroy(n->s2);
  if (n->ev_fork) hipEventDestroy(n->ev_fork);
  if (n->ev_den) hipEventDestroy(n->ev_den);
  if (n->ev_num) hipEventDestroy(n->ev_num);
  if (n->ev_s3) hipEventDestroy(n->ev_s3);
  if (n->ev_fin0) hipEventDestroy(n->ev_fin0);
  if (n->ev_fin) hipEventDestroy(n->ev_fin);
  if (n->s3) hipStreamDestroy(n->s3);
  for (hipEvent_t e : {n->ev_pg[0], n->ev_pg[1], n->ev_pg[2], n->ev_pg[3], n->ev_pg_in, n->ev_early_in, n->ev_early, n->ev_comm, n->ev_den_rec})
    if (e) hipEventDestroy(e);
  if (n->s4) hipStreamDestroy(n->s4);
  if (n->s5) hipStreamDestroy(n->s5);
  rows_gemm_group_destroy(n->early_launch);
  planes_split_group_destroy(n->wsplit_group);
  for (hipEvent_t e : n->ev_phase)
    if (e) hipEventDestroy(e);
  upd_group_destroy(n->upd);
  delete n;
}

long long tdnnf_net_num_params(const tdnnf_net *n) { return n ? n->num_params : 0; }
int tdnnf_net_num_components(const tdnnf_net *n) { return n ? (int)n->comps.size() : 0; }

int tdnnf_net_component_info(const tdnnf_net *n, int i, char *name_out, long long *begin, int *rows, int *cols, int *has_bias,
                             float *lr_factor, float *l2, float *max_change, float *orthonormal) {
  TDNNF_REQUIRE(n && i >= 0 && i < (int)n->comps.size(), "net_component_info: bad index");
  const CompDesc &c = n->comps[i];
  if (name_out) snprintf(name_out, 64, "%s", c.name.c_str());
  if (begin) *begin = c.begin;
  if (rows) *rows = c.rows;
  if (cols) *cols = c.cols;
  if (has_bias) *has_bias = c.has_bias;
  if (lr_factor) *lr_factor = c.lr_factor;
  if (l2) *l2 = c.l2;
  if (max_change) *max_change = c.max_change;
  if (orthonormal) *orthonormal = c.orthonormal;
  return TDNNF_OK;
}

// model statistics outside the parameter vector: [count, sum[D], sumsq[D]] of every BatchNorm and
// [count, value_sum[D], deriv_sum[D]] of every ReLU, in network order
static void stat_blocks(const tdnnf_net *n, std::vector<std::pair<double *, int>> &out) {  // (pointer, number of doubles)
  const int Hd = n->cfg.hidden_dim, S = n->cfg.prefinal_small_dim;
  auto bn = [&](double *p, int D) { out.push_back({p, 1 + 2 * D}); };
  auto relu = [&](double *p, int D) { out.push_back({p, 2 + 3 * D}); };
  bn(n->t1_bn_stats, Hd);
  relu(n->t1_relu_stats, Hd);
  for (auto &L : n->layers) {
    bn(L.bn_stats, Hd);
    relu(L.relu_stats, Hd);
  }
  for (int h = 0; h < 2; h++) {
    bn(n->head[h].bn1_stats, Hd);
    relu(n->head[h].relu_stats, Hd);
    bn(n->head[h].bn2_stats, S);
  }
}
long long tdnnf_net_stats_size(const tdnnf_net *n) {
  if (!n) return 0;
  std::vector<std::pair<double *, int>> b;
  stat_blocks(n, b);
  long long t = 0;
  for (auto &x : b) t += x.second;
  return t;
}
int tdnnf_net_get_stats(const tdnnf_net *n, double *host_out, tdnnf_stream stream) {
  TDNNF_REQUIRE(n && host_out, "net_get_stats: null argument");
  std::vector<std::pair<double *, int>> b;
  stat_blocks(n, b);
  TDNNF_HIP(hipStreamSynchronize((hipStream_t)stream));
  for (auto &x : b) {
    TDNNF_HIP(hipMemcpy(host_out, x.first, sizeof(double) * x.second, hipMemcpyDeviceToHost));
    host_out += x.second;
  }
  return TDNNF_OK;
}
int tdnnf_net_set_stats(tdnnf_net *n, const double *host_in, tdnnf_stream stream) {
  TDNNF_REQUIRE(n && host_in, "net_set_stats: null argument");
  std::vector<std::pair<double *, int>> b;
  stat_blocks(n, b);
  {  // oderiv_count of every ReLU block ([count, value_sum[D], deriv_sum[D], oderiv_count, oderiv_sumsq[D]]); stat_blocks() order:
     // tdnn1 (bn, relu), every tdnnf layer (bn, relu), both heads (bn1, relu, bn2)
    std::vector<char> &nz = *n->oderiv_nonzero;
    nz.assign(n->cfg.num_layers + 3, 0);
    std::vector<int> is_relu = {0, 1};
    for (int l = 0; l < n->cfg.num_layers; l++) is_relu.insert(is_relu.end(), {0, 1});
    for (int h = 0; h < 2; h++) is_relu.insert(is_relu.end(), {0, 1, 0});
    const double *p = host_in;
    int k = 0;
    for (size_t i = 0; i < b.size(); i++) {
      if (i < is_relu.size() && is_relu[i]) {
        const int D = (b[i].second - 2) / 3;
        nz[k++] = p[1 + 2 * D] != 0.0;
      }
      p += b[i].second;
    }
  }
  TDNNF_HIP(hipStreamSynchronize((hipStream_t)stream));
  for (auto &x : b) {
    TDNNF_HIP(hipMemcpy(x.first, host_in, sizeof(double) * x.second, hipMemcpyHostToDevice));
    host_in += x.second;
  }
  return TDNNF_OK;
}

int tdnnf_net_set_dropout_proportion(tdnnf_net *n, float proportion) {
  TDNNF_REQUIRE(n && proportion >= 0.f && proportion <= 0.5f, "net_set_dropout_proportion: proportion must be in [0, 0.5] (continuous masks: scale in [1 - 2p, 1 + 2p])");
  TDNNF_REQUIRE(proportion == 0.f || n->dropout_masks, "net_set_dropout_proportion: the net was created without use_dropout (or in cv-update mode)");
  n->dropout_proportion = proportion;
  return TDNNF_OK;
}

int tdnnf_net_set_temperature_proportion(tdnnf_net *n, float proportion) {
  TDNNF_REQUIRE(n && proportion > 0.f, "net_set_temperature_proportion: proportion must be > 0");
  n->cfg.darts_temp_proportion = proportion;
  n->cfg.bn_temp_proportion = proportion;
  return TDNNF_OK;
}

// NameMatchesPattern (UPSTREAM, used by every edit directive of nnet-utils.cc:1166-1415): '*' matches any run of characters
static bool name_matches(const char *name, const char *pat) {
  if (*pat == 0) return *name == 0;
  if (*pat == '*') {
    for (const char *p = name;; p++) {
      if (name_matches(p, pat + 1)) return true;
      if (*p == 0) return false;
    }
  }
  return *name == *pat && name_matches(name + 1, pat + 1);
}

int tdnnf_net_set_batchnorm_sync(tdnnf_net *n, TDNNF_ALLREDUCE_FN *allreduce, void *ctx, int world_size) {
  TDNNF_REQUIRE(n && world_size >= 1, "net_set_batchnorm_sync: bad arguments");
  n->bn_sync.fn = allreduce;
  n->bn_sync.ctx = ctx;
  n->bn_sync.world = world_size;
  return TDNNF_OK;
}

int tdnnf_net_set_learning_rate_factor(tdnnf_net *n, const char *name_pattern, float factor, int *num_set) {
  TDNNF_REQUIRE(n && name_pattern && factor >= 0.f, "net_set_learning_rate_factor: bad arguments (the factor must be >= 0)");
  int cnt = 0;
  for (auto &cd : n->comps)
    if (cd.updatable && name_matches(cd.name.c_str(), name_pattern)) {
      cd.lr_factor = factor;
      cnt++;
    }
  if (num_set) *num_set = cnt;
  return TDNNF_OK;
}

int tdnnf_net_component_num_alpha(const tdnnf_net *n, int i) {
  return n && i >= 0 && i < (int)n->comps.size() ? n->comps[i].num_alpha : 0;
}
int tdnnf_net_num_random_draws(const tdnnf_net *n) { return n ? n->num_draws : 0; }
int tdnnf_net_set_random_draws(tdnnf_net *n, const float *draws) {
  TDNNF_REQUIRE(n && (draws || n->num_draws == 0), "net_set_random_draws: null argument");
  n->draws = draws;
  return TDNNF_OK;
}

int tdnnf_net_input_frames(const tdnnf_net *n, int *num_t_in, int *first_t) {
  TDNNF_REQUIRE(n, "net_input_frames: null net");
  if (num_t_in) *num_t_in = n->g_feat.n;
  if (first_t) *first_t = n->g_feat.t0;
  return TDNNF_OK;
}

int tdnnf_net_set_buffers(tdnnf_net *n, float *params, float *grads) {
  TDNNF_REQUIRE(n && params && grads && ((uintptr_t)params & 15) == 0 && ((uintptr_t)grads & 15) == 0,
                "net_set_buffers: buffers must be non-null and 16-byte aligned");
  n->params = params;
  n->grads = grads;
  return TDNNF_OK;
}

int tdnnf_net_num_grad_buckets(const tdnnf_net *n) { return n ? (int)n->buckets.size() : 0; }
int tdnnf_net_grad_bucket(const tdnnf_net *n, int i, long long *begin, long long *end) {
  TDNNF_REQUIRE(n && i >= 0 && i < (int)n->buckets.size(), "net_grad_bucket: bad index");
  if (begin) *begin = n->buckets[i].begin;
  if (end) *end = n->buckets[i].end;
  return TDNNF_OK;
}
int tdnnf_net_wait_grad_bucket(const tdnnf_net *n, int i, tdnnf_stream stream) {
  TDNNF_REQUIRE(n && i >= 0 && i < (int)n->buckets.size(), "net_wait_grad_bucket: bad index");
  TDNNF_HIP(hipStreamWaitEvent((hipStream_t)stream, n->buckets[i].ready, 0));
  return TDNNF_OK;
}

int tdnnf_net_set_capture(tdnnf_net *n, int on) {
  TDNNF_REQUIRE(n, "net_set_capture: null net");
  n->capture_on = on != 0;
  return TDNNF_OK;
}

int tdnnf_net_activation_dims(const tdnnf_net *n, const char *name, int *rows, int *cols) {
  TDNNF_REQUIRE(n && name, "net_activation_dims: null argument");
  for (auto &kv : n->named)
    if (kv.first == name) {
      if (rows) *rows = kv.second.rows;
      if (cols) *cols = kv.second.cols;
      return TDNNF_OK;
    }
  set_error("net_activation_dims: unknown activation '%s'", name);
  return TDNNF_EINVAL;
}

int tdnnf_net_get_activation(const tdnnf_net *n, const char *name, tdnnf_mat *out, tdnnf_stream stream) {
  TDNNF_REQUIRE(n && name && mat_ok(out), "net_get_activation: bad argument");
  for (auto &kv : n->named)
    if (kv.first == name) {
      TDNNF_REQUIRE(out->rows == kv.second.rows && out->cols == kv.second.cols, "net_get_activation: %s is %d x %d", name,
                    kv.second.rows, kv.second.cols);
      return tdnnf_sum_scaled(&kv.second, 1.0f, nullptr, 0.f, out, stream);
    }
  set_error("net_get_activation: unknown activation '%s'", name);
  return TDNNF_EINVAL;
}

int tdnnf_net_update(tdnnf_net *n, float lr, float l2_scale, long long step, tdnnf_stream stream) {
  TDNNF_REQUIRE(n && n->params && n->grads, "net_update: call net_set_buffers first");
  TDNNF_REQUIRE(lr >= 0.f && l2_scale >= 0.f, "net_update: learning rate and l2 scale must be >= 0 (nnet-utils.cc:2240)");
  TraceRange trace_update("tdnnf_net_update");
  hipStream_t s = (hipStream_t)stream;
  CK(phase_mark(n, 6, s));
  const int nc = (int)n->comps.size();
  UpdTable tb;
  memset(&tb, 0, sizeof(tb));
  std::vector<long long> begin(nc + 1);
  std::vector<float> mc(nc);
  for (int i = 0; i < nc; i++) {
    const CompDesc &c = n->comps[i];
    begin[i] = tb.begin[i] = c.begin;
    const float lrc = lr * c.lr_factor;
    tb.lr[i] = lrc;
    tb.l2coef[i] = -2.0f * l2_scale * lrc * c.l2;  // ApplyL2Regularization, nnet-utils.cc:2241
    mc[i] = c.max_change;
  }
  begin[nc] = tb.begin[nc] = n->num_params;
  // component i owns [begin[i], begin[i+1]) including alignment padding (padding stays zero).  delta = lr g + l2 theta, max-change and the
  // update as three launches over all components (optim_group.hip)
  if (!n->upd || upd_group_params(n->upd) != n->params) {
    upd_group_destroy(n->upd);
    n->upd = nullptr;
    std::vector<UpdComp> uc(nc);
    for (int i = 0; i < nc; i++) {
      const CompDesc &c = n->comps[i];
      uc[i] = UpdComp{begin[i], begin[i + 1], c.rows, c.cols, c.orthonormal};
    }
    CK(upd_group_create(uc, n->params, &n->upd));
  }
  CK(upd_group_step(n->upd, n->params, n->grads, tb.lr, tb.l2coef, mc.data(), n->cfg.max_param_change, s));
  // ScaleBatchnormStats
  if (n->cfg.batchnorm_stats_scale != 1.0f && !n->cfg.cv_update) {  // (BatchNormTestComponents are not scaled)
    const int Hd = n->cfg.hidden_dim, S = n->cfg.prefinal_small_dim;
    ScaleTable tb;
    memset(&tb, 0, sizeof(tb));
    int nb = 0, maxn = 0;
    auto sc = [&](double *st, int D) {
      if (nb < 48) {
        tb.p[nb] = st;
        tb.n[nb] = 1 + 2 * D;
        maxn = std::max(maxn, 1 + 2 * D);
        nb++;
      }
    };
    sc(n->t1_bn_stats, Hd);
    for (auto &L : n->layers) sc(L.bn_stats, Hd);
    for (int h = 0; h < 2; h++) {
      sc(n->head[h].bn1_stats, Hd);
      sc(n->head[h].bn2_stats, S);
    }
    TDNNF_REQUIRE(nb == (int)n->layers.size() + 5, "net_update: too many BatchNorm components for one launch");
    hipLaunchKernelGGL(scale_doubles_kernel, dim3((maxn + 255) / 256, nb), dim3(256), 0, s, tb, (double)n->cfg.batchnorm_stats_scale);
  }
  // ConstrainOrthonormal: each constrained component with probability 1/4 (nnet-utils.cc:1062); the ones chosen this minibatch run
  // together as grouped launches (tall matrices -- none in the recipes' graphs -- keep the per-component path on the transpose)
  std::vector<int> chosen;
  for (int i = 0; i < nc; i++) {
    const CompDesc &c = n->comps[i];
    if (c.orthonormal == 0.f) continue;
    if (::tdnnf::tdnnf_decision((unsigned long long)step, 2 * (unsigned long long)i + 1) % 4 != 0) continue;  // RandInt(0,3) != 0
    if (upd_group_can_ortho(n->upd, i)) {
      chosen.push_back(i);
    } else if (c.rows <= c.cols) {
      CK(tdnnf_constrain_orthonormal(c.orthonormal, n->params + c.begin, c.rows, c.cols, c.cols, n->ws, n->ws_bytes, s));
    } else {  // tall matrix: constrain the transpose (nnet-utils.cc:1068-1075)
      TDNNF_REQUIRE(n->orthoT, "net_update: no transpose buffer for %s", c.name.c_str());
      const long long total = (long long)c.rows * c.cols;
      hipLaunchKernelGGL(transpose_kernel, dim3(grid_for(total, 256)), dim3(256), 0, s, n->params + c.begin, c.rows, c.cols, n->orthoT);
      CK(tdnnf_constrain_orthonormal(c.orthonormal, n->orthoT, c.cols, c.rows, c.rows, n->ws, n->ws_bytes, s));
      hipLaunchKernelGGL(transpose_kernel, dim3(grid_for(total, 256)), dim3(256), 0, s, n->orthoT, c.cols, c.rows, n->params + c.begin);
    }
  }
  if (!chosen.empty()) CK(upd_group_ortho(n->upd, chosen, s));
  CK(phase_mark(n, 7, s));
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

}  // extern "C"
