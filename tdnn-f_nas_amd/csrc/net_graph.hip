// net_graph.hip -- the chain trainer's network for the TDNN-F graphs of the reference recipes, as far as it can be said without the
// device (no HIP call here): config checks, time grids, TdnnComponent indexes, the component list with its random-draw plan, the cv-update
// learning-rate factors, the "same model as the primary" check, the gradient-bucket ranges, and the lists of net_model.h.
//
// Graph: /root/reference/local/chain_NAS/run_tdnn_fbk_40_iv_sp_7q.sh:160-186; one tdnnf-layer =
// steps/libs/nnet3/xconfig/composite_layers.py:135-215, prefinal-layer :1283-1331.
//
// Time bookkeeping replaces the nnet3 compiler for these graphs: every layer's output lives on a regular
// grid (t0, step, n) in t-major row order (row = k*B + b), derived backwards from the output grid
// (0, 3, T/3) exactly as the compiler's dependency analysis would (tdnnf4.linear is computed on the
// padded step-1 grid, as TdnnComponent::ReorderIndexes pads it).
#include <string.h>

#include <string>
#include <vector>

#include "common.h"
#include "net_model.h"

namespace tdnnf {
namespace {

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

// gradient buckets: whole layers, cut from the top of the flat buffer downwards (= the order backward finishes them)
void bucket_ranges(tdnnf_net *n) {
  const long long target = 4LL << 20;  // >= 16 MB of fp32 per collective (xGMI rings want large messages), layers kept whole
  auto first_comp_of_layer = [&](int l) { return n->layers[l].c_arch >= 0 ? n->layers[l].c_arch : n->layers[l].lin.comp; };
  long long end = n->num_params;
  n->buckets.push_back(tdnnf_net::GradBucket{n->comps[n->c_prefinal_l].begin, end, -2});
  end = n->buckets.back().begin;
  for (int l = n->cfg.num_layers - 1; l >= 0; l--) {
    const long long begin = n->comps[first_comp_of_layer(l)].begin;
    if (end - begin >= target) {
      n->buckets.push_back(tdnnf_net::GradBucket{begin, end, l});
      end = begin;
    }
  }
  n->buckets.push_back(tdnnf_net::GradBucket{0, end, -1});
}

}  // namespace

std::vector<StatBlock> stat_blocks(const tdnnf_net *cn) {
  tdnnf_net *n = const_cast<tdnnf_net *>(cn);  // (for `slot`; nothing is written here)
  const int Hd = n->cfg.hidden_dim, S = n->cfg.prefinal_small_dim;
  std::vector<StatBlock> out;
  auto bn = [&](const std::string &name, double **slot, int D, int head = -1) { out.push_back({name, slot, D, false, head}); };
  auto relu = [&](const std::string &name, double **slot, int D, int head = -1) { out.push_back({name, slot, D, true, head}); };
  bn("tdnn1.batchnorm", &n->t1_bn_stats, Hd);
  relu("tdnn1.relu", &n->t1_relu_stats, Hd);
  for (size_t l = 0; l < n->layers.size(); l++) {
    const std::string p = "tdnnf" + std::to_string(l + 2);
    bn(p + ".batchnorm", &n->layers[l].bn_stats, Hd);
    relu(p + ".relu", &n->layers[l].relu_stats, Hd);
  }
  for (int h = 0; h < 2; h++) {
    const std::string p = std::string("prefinal-") + head_name(h);
    bn(p + ".batchnorm1", &n->head[h].bn1_stats, Hd, h);
    relu(p + ".relu", &n->head[h].relu_stats, Hd, h);
    bn(p + ".batchnorm2", &n->head[h].bn2_stats, S, h);
  }
  return out;
}

std::vector<WeightComp> weight_comps(const tdnnf_net *n) {
  const int No = n->Tout * n->B;
  std::vector<WeightComp> out;
  out.push_back({n->tdnn1.comp, 1, n->tdnn1.rows_out});
  for (auto &L : n->layers) {
    out.push_back({L.lin.comp, L.lin.K, L.lin.rows_out});
    out.push_back({L.aff.comp, L.aff.K, L.aff.rows_out});
  }
  out.push_back({n->c_prefinal_l, 1, No});
  for (int h = 0; h < 2; h++)
    for (int comp : {n->head[h].c_affine, n->head[h].c_linear, n->head[h].c_output}) out.push_back({comp, 1, No});
  return out;
}

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

void layer_taps(const tdnnf_net_config &c, const TdnnfLayer &L, std::vector<int> *lin, std::vector<int> *aff) {
  lin->clear();
  aff->clear();
  if (const int K = c.darts_num_offsets; K >= 2) {
    for (int i = 0; i < K; i++) {
      lin->push_back(-(K - 1) + i);
      aff->push_back(i);
    }
  } else {
    *lin = L.left > 0 ? std::vector<int>{-L.left, 0} : std::vector<int>{0};
    *aff = L.right > 0 ? std::vector<int>{0, L.right} : std::vector<int>{0};
  }
}

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

int net_check_config(const tdnnf_net_config &c) {
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
  return TDNNF_OK;
}

int net_describe(tdnnf_net *n) {
  const tdnnf_net_config &c = n->cfg;
  n->B = c.num_sequences;
  n->T = c.frames_per_chunk;
  n->Tout = c.frames_per_chunk / c.frame_subsampling;
  const int B = n->B, Hd = c.hidden_dim, S = c.prefinal_small_dim, P = c.num_pdfs, lda_dim = 3 * c.feat_dim + c.ivector_dim;
  // ---- grids, derived backwards from the output grid
  CK(net_layer_grids(c, n->Tout, n->layers, &n->g_lda));
  TDNNF_REQUIRE(n->g_lda.step == 1, "net_create: the first tdnnf layers must run at the input frame rate");
  n->g_feat = feat_grid(n->g_lda);
  // ---- components, in nnet3 config order
  n->c_lda = add_comp(n, "lda", lda_dim, lda_dim, 1, 0.f, 0.f, 0.f, 0.f);
  n->comps[n->c_lda].updatable = false;
  const int c_t1 = add_comp(n, "tdnn1.affine", Hd, lda_dim, 1, 1.f, c.l2_hidden, c.max_change_hidden, 0.f);
  make_tdnn(&n->tdnn1, c_t1, lda_dim, Hd, std::vector<int>{0}, n->g_lda, n->g_lda, B);
  for (int l = 0; l < c.num_layers; l++) {
    TdnnfLayer &L = n->layers[l];
    const bool darts = c.darts_num_offsets >= 2;
    const int K = darts ? c.darts_num_offsets : 0;  // taps of a searched component
    std::vector<int> lin_off, aff_off;
    layer_taps(c, L, &lin_off, &aff_off);
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
  if (c.use_dropout && !c.cv_update) n->num_draws += (c.num_layers + 1) * B * Hd;  // one B x Hd mask per GeneralDropoutComponent
  n->c_prefinal_l = add_comp(n, "prefinal-l", S, Hd, 0, 1.f, c.l2_hidden, c.max_change_hidden, -1.0f);
  for (int h = 0; h < 2; h++) {
    char nm[64];
    snprintf(nm, sizeof(nm), "prefinal-%s.affine", head_name(h));
    n->head[h].c_affine = add_comp(n, nm, Hd, S, 1, 1.f, c.l2_hidden, c.max_change_hidden, 0.f);
    snprintf(nm, sizeof(nm), "prefinal-%s.linear", head_name(h));
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
  bucket_ranges(n);
  return TDNNF_OK;
}

// another minibatch shape of the same model: same components, so that it can use the primary's parameters, preconditioners and statistics
int net_same_model(const tdnnf_net *n, const tdnnf_net *primary) {
  bool same = primary->comps.size() == n->comps.size() && primary->num_params == n->num_params &&
              (primary->cfg.use_natural_gradient != 0) == (n->cfg.use_natural_gradient != 0) && primary->cfg.cv_update == n->cfg.cv_update;
  for (size_t i = 0; same && i < n->comps.size(); i++)
    same = primary->comps[i].name == n->comps[i].name && primary->comps[i].rows == n->comps[i].rows && primary->comps[i].cols == n->comps[i].cols &&
           primary->comps[i].begin == n->comps[i].begin;
  TDNNF_REQUIRE(same, "net_create_shared: the configuration describes another model than the primary net's");
  return TDNNF_OK;
}

}  // namespace tdnnf
