// chain_graph.hip -- host only: builds the denominator graph's three SELL-64 tables and the supervision's per-state arc lists
// (chain_types.h), for a wide supervision also its numerator scratch and its per-frame arcs ordered by pdf, and copies them to the device.
#include <string.h>

#include <algorithm>
#include <vector>

#include "chain_types.h"

namespace tdnnf {
namespace {

template <class T>
int to_device(const std::vector<T> &v, T **out) {
  *out = nullptr;
  if (v.empty()) {
    TDNNF_HIP(hipMalloc((void **)out, sizeof(T)));
    return TDNNF_OK;
  }
  TDNNF_HIP(hipMalloc((void **)out, sizeof(T) * v.size()));
  TDNNF_HIP(hipMemcpy(*out, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
  return TDNNF_OK;
}

// rows[r] = list of (key, prob); builds SELL-64 over rows sorted by descending degree (stable)
// init (may be null): initial probabilities indexed by the low 16 bits of the key (the arc's source state), for arc4.z
int build_sell(int nrows, const std::vector<std::vector<std::pair<unsigned, float>>> &rows, const std::vector<float> *init, tdnnf_den_graph::Sell *out) {
  const int ns = (nrows + 63) / 64;
  std::vector<int> order(nrows);
  for (int r = 0; r < nrows; r++) order[r] = r;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return rows[a].size() > rows[b].size(); });
  std::vector<int> base(ns + 1, 0);
  for (int k = 0; k < ns; k++) base[k + 1] = base[k] + (int)rows[order[64 * k]].size() * 64;
  std::vector<unsigned> rowid((size_t)ns * 64, 0xffffffffu);
  std::vector<uint2> arc(base[ns], make_uint2(0u, 0u));  // padding: state 0 / pdf 0 with prob 0
  std::vector<uint4> arc4(base[ns], make_uint4(0u, 0u, 0u, 0u));
  // The order of a row's arcs is free (a sum).  The j-th arcs of a slice's 64 rows are read by one wave instruction and become two LDS gathers
  // (the two 16-bit halves of the key index state / pdf vectors): 64 random addresses put 4-5 on the worst of 64 banks.  Greedy per position: every
  // row takes, among its arcs not placed yet, the one whose two banks are least used at this position so far (half a wave -- 32 lanes -- is what the
  // LDS serves at once).  The persistent recursions are bound by these gathers, not by the arc loads (docs/experiments.md r4-i).
  std::vector<std::vector<std::pair<unsigned, float>>> placed(nrows);
  for (int k = 0; k < ns; k++) {
    const int w = (base[k + 1] - base[k]) / 64;
    std::vector<std::vector<char>> used(64);
    for (int l = 0; l < 64 && 64 * k + l < nrows; l++) used[l].assign(rows[order[64 * k + l]].size(), 0);
    for (int j = 0; j < w; j++) {
      int load[2][2][64];  // [half-wave][which key half][bank]
      memset(load, 0, sizeof(load));
      for (int l = 0; l < 64 && 64 * k + l < nrows; l++) {
        const auto &src = rows[order[64 * k + l]];
        int best = -1, best_cost = 1 << 30;
        for (size_t c = 0; c < src.size(); c++) {
          if (used[l][c]) continue;
          const int cost = load[l >> 5][0][src[c].first & 63u] + load[l >> 5][1][(src[c].first >> 16) & 63u];
          if (cost < best_cost) {
            best_cost = cost;
            best = (int)c;
          }
        }
        if (best < 0) continue;  // (this row is shorter than the slice: padding from here on)
        used[l][best] = 1;
        load[l >> 5][0][src[best].first & 63u]++;
        load[l >> 5][1][(src[best].first >> 16) & 63u]++;
        placed[order[64 * k + l]].push_back(src[best]);
      }
    }
  }
  for (int s = 0; s < nrows; s++) {
    const int r = order[s];
    rowid[s] = (unsigned)r;
    for (size_t j = 0; j < placed[r].size(); j++) {
      unsigned bits;
      memcpy(&bits, &placed[r][j].second, 4);
      arc[base[s / 64] + j * 64 + s % 64] = make_uint2(placed[r][j].first, bits);
      const float ip = init ? placed[r][j].second * (*init)[placed[r][j].first & 0xffffu] : 0.f;
      unsigned ibits;
      memcpy(&ibits, &ip, 4);
      arc4[base[s / 64] + j * 64 + s % 64] = make_uint4(placed[r][j].first, bits, ibits, 0u);
    }
  }
  out->nrows = nrows;
  out->nslices = ns;
  out->entries = base[ns];
  for (int G = 0; G <= 8; G++) {
    out->mw_max_arcs[G] = 0;
    if (G != 2 && G != 4 && G != 8) continue;
    for (int g = 0; g < G; g++) {
      int own = 0;
      for (int k = g; k < ns; k += G) own += base[k + 1] - base[k];
      out->mw_max_arcs[G] = std::max(out->mw_max_arcs[G], own);
    }
  }
  int rc;
  if ((rc = to_device(base, &out->base))) return rc;
  if ((rc = to_device(rowid, &out->row))) return rc;
  if ((rc = to_device(arc4, &out->arc4))) return rc;
  return to_device(arc, &out->arc);
}

}  // namespace
}  // namespace tdnnf

using namespace tdnnf;

extern "C" {

int tdnnf_den_graph_create(int H, int A, int P, const int *src, const int *dst, const int *pdf, const float *prob,
                           const float *initial_probs, int start_state, tdnnf_den_graph **out) {
  TDNNF_REQUIRE(out && H > 0 && A > 0 && P > 0 && src && dst && pdf && prob, "den_graph_create: bad arguments");
  TDNNF_REQUIRE(H <= 65535 && P <= 65535, "den_graph_create: num_states and num_pdfs must be <= 65535 (16-bit packed arcs)");
  for (int a = 0; a < A; a++)
    TDNNF_REQUIRE(src[a] >= 0 && src[a] < H && dst[a] >= 0 && dst[a] < H && pdf[a] >= 0 && pdf[a] < P && prob[a] >= 0,
                  "den_graph_create: arc %d out of range", a);
  std::vector<float> init(H);
  if (initial_probs) {
    init.assign(initial_probs, initial_probs + H);
  } else {  // DenominatorGraph::SetInitialProbs: 100-step average occupancy of the row-normalised graph
    TDNNF_REQUIRE(start_state >= 0 && start_state < H, "den_graph_create: bad start state");
    std::vector<double> norm(H, 0.0), cur(H, 0.0), nxt(H), avg(H, 0.0);
    for (int a = 0; a < A; a++) norm[src[a]] += prob[a];
    cur[start_state] = 1.0;
    for (int it = 0; it < 100; it++) {
      for (int h = 0; h < H; h++) avg[h] += cur[h] / 100;
      std::fill(nxt.begin(), nxt.end(), 0.0);
      for (int a = 0; a < A; a++)
        if (norm[src[a]] > 0) nxt[dst[a]] += cur[src[a]] * prob[a] / norm[src[a]];
      cur.swap(nxt);
    }
    for (int h = 0; h < H; h++) init[h] = (float)avg[h];
  }
  tdnnf_den_graph *g = new tdnnf_den_graph();
  memset(g, 0, sizeof(*g));
  g->H = H;
  g->A = A;
  g->P = P;
  std::vector<std::vector<std::pair<unsigned, float>>> bd(H), bs(H), bp(P);
  for (int a = 0; a < A; a++) {
    bd[dst[a]].push_back({(unsigned)src[a] | ((unsigned)pdf[a] << 16), prob[a]});
    bs[src[a]].push_back({(unsigned)dst[a] | ((unsigned)pdf[a] << 16), prob[a]});
    bp[pdf[a]].push_back({(unsigned)src[a] | ((unsigned)dst[a] << 16), prob[a]});
  }
  int rc;
  if ((rc = build_sell(H, bd, &init, &g->by_dst)) || (rc = build_sell(H, bs, nullptr, &g->by_src)) || (rc = build_sell(P, bp, &init, &g->by_pdf)) ||
      (rc = to_device(init, &g->init))) {
    tdnnf_den_graph_destroy(g);
    return rc;
  }
  double sd = 0;  // a double sum in index order, rounded to float once
  for (int h = 0; h < H; h++) sd += init[h];
  g->init_sum = (float)sd;
  *out = g;
  return TDNNF_OK;
}

void tdnnf_den_graph_destroy(tdnnf_den_graph *g) {
  if (!g) return;
  tdnnf_den_graph::Sell *t[3] = {&g->by_dst, &g->by_src, &g->by_pdf};
  for (auto *x : t) {
    hipFree(x->base);
    hipFree(x->row);
    hipFree(x->arc);
    hipFree(x->arc4);
  }
  hipFree(g->init);
  delete g;
}

int tdnnf_supervision_create(int B, int T, const int *seq_state_begin, const int *seq_arc_begin, const int *state_time,
                             const float *final_logprob, const int *arc_src, const int *arc_dst, const int *arc_pdf,
                             const float *arc_logprob, float weight, tdnnf_supervision **out) {
  TDNNF_REQUIRE(out && B > 0 && T > 0 && seq_state_begin && seq_arc_begin && state_time && final_logprob && arc_src &&
                    arc_dst && arc_pdf && arc_logprob,
                "supervision_create: bad arguments");
  const int NS = seq_state_begin[B], NA = seq_arc_begin[B];
  std::vector<int> fsb((size_t)B * (T + 2), 0);
  int max_states = 0;
  for (int s = 0; s < B; s++) {
    const int s0 = seq_state_begin[s], s1 = seq_state_begin[s + 1];
    max_states = std::max(max_states, s1 - s0);
    TDNNF_REQUIRE(s1 > s0 && state_time[s0] == 0, "supervision_create: sequence %d must start with its time-0 start state", s);
    int st = s0;
    for (int t = 0; t <= T + 1; t++) {
      while (st < s1 && state_time[st] < t) st++;
      fsb[(size_t)s * (T + 2) + t] = st;
    }
    for (int i = s0 + 1; i < s1; i++)
      TDNNF_REQUIRE(state_time[i] >= state_time[i - 1] && state_time[i] <= T, "supervision_create: states must be sorted by time");
    TDNNF_REQUIRE(fsb[(size_t)s * (T + 2) + 1] == s0 + 1, "supervision_create: exactly one time-0 state per sequence");
    for (int a = seq_arc_begin[s]; a < seq_arc_begin[s + 1]; a++)
      TDNNF_REQUIRE(arc_src[a] >= s0 && arc_src[a] < s1 && arc_dst[a] >= s0 && arc_dst[a] < s1 && arc_pdf[a] >= 0 &&
                        state_time[arc_dst[a]] == state_time[arc_src[a]] + 1,
                    "supervision_create: arc %d must advance exactly one frame inside its sequence", a);
  }
  std::vector<int> in_begin(NS + 1, 0), out_begin(NS + 1, 0);
  for (int a = 0; a < NA; a++) {
    in_begin[arc_dst[a] + 1]++;
    out_begin[arc_src[a] + 1]++;
  }
  for (int i = 0; i < NS; i++) {
    in_begin[i + 1] += in_begin[i];
    out_begin[i + 1] += out_begin[i];
  }
  std::vector<int> in_src(NA), in_pdf(NA), out_dst(NA), out_pdf(NA), ipos(in_begin.begin(), in_begin.end() - 1),
      opos(out_begin.begin(), out_begin.end() - 1);
  std::vector<float> in_lp(NA), out_lp(NA);
  for (int a = 0; a < NA; a++) {  // stable: original arc order within each state
    int i = ipos[arc_dst[a]]++, o = opos[arc_src[a]]++;
    in_src[i] = arc_src[a];
    in_pdf[i] = arc_pdf[a];
    in_lp[i] = arc_logprob[a];
    out_dst[o] = arc_dst[a];
    out_pdf[o] = arc_pdf[a];
    out_lp[o] = arc_logprob[a];
  }
  tdnnf_supervision *sp = new tdnnf_supervision();
  memset(sp, 0, sizeof(*sp));
  sp->B = B;
  sp->T = T;
  sp->num_states = NS;
  sp->num_arcs = NA;
  sp->weight = weight;
  sp->max_states_per_seq = max_states;
  // A supervision wider than the workspace's numerator scratch (chain_den.hip chain_bufs) owns its log alpha / log beta, and carries what
  // num_wide_kernels.h walks: the arcs that leave each frame ordered by pdf.  A narrow one gets the latter only when option num_form asks
  // for the wide form at creation (A/B runs, tests).
  sp->wide = (long long)NS > (long long)B * 4 * (T + 1);
  std::vector<int> pf_src, pf_dst, pf_pdf, pf_t;
  std::vector<float> pf_lp;
  const bool tables = sp->wide || options().num_form == 2;
  for (int s = 0; s < B; s++)
    for (int t = 0; t <= T; t++) {
      const int f0 = fsb[(size_t)s * (T + 2) + t], f1 = fsb[(size_t)s * (T + 2) + t + 1];
      sp->max_states_per_frame = std::max(sp->max_states_per_frame, f1 - f0);
      sp->max_arcs_per_frame = std::max(sp->max_arcs_per_frame, out_begin[f1] - out_begin[f0]);
    }
  if (tables) {
    pf_src.resize(NA);
    pf_dst.resize(NA);
    pf_pdf.resize(NA);
    pf_t.resize(NA);
    pf_lp.resize(NA);
    std::vector<int> src_of(NA), order;
    for (int st = 0; st < NS; st++)
      for (int o = out_begin[st]; o < out_begin[st + 1]; o++) src_of[o] = st;
    for (int s = 0; s < B; s++)
      for (int t = 0; t < T; t++) {
        const int a0 = out_begin[fsb[(size_t)s * (T + 2) + t]], a1 = out_begin[fsb[(size_t)s * (T + 2) + t + 1]];
        order.resize(a1 - a0);
        for (int o = a0; o < a1; o++) order[o - a0] = o;
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return out_pdf[x] < out_pdf[y]; });
        for (int o = a0; o < a1; o++) {
          const int from = order[o - a0];
          pf_src[o] = src_of[from];
          pf_dst[o] = out_dst[from];
          pf_pdf[o] = out_pdf[from];
          pf_t[o] = t;
          pf_lp[o] = out_lp[from];
        }
      }
  }
  std::vector<int> ssb(seq_state_begin, seq_state_begin + B + 1), stime(state_time, state_time + NS);
  std::vector<float> fin(final_logprob, final_logprob + NS);
  int rc;
  if ((rc = to_device(ssb, &sp->seq_state_begin)) || (rc = to_device(stime, &sp->state_time)) ||
      (rc = to_device(fin, &sp->final_logprob)) || (rc = to_device(in_begin, &sp->in_begin)) ||
      (rc = to_device(in_src, &sp->in_src)) || (rc = to_device(in_pdf, &sp->in_pdf)) || (rc = to_device(in_lp, &sp->in_lp)) ||
      (rc = to_device(out_begin, &sp->out_begin)) || (rc = to_device(out_dst, &sp->out_dst)) ||
      (rc = to_device(out_pdf, &sp->out_pdf)) || (rc = to_device(out_lp, &sp->out_lp)) ||
      (rc = to_device(fsb, &sp->frame_state_begin)) || (rc = to_device(std::vector<double>(kFinishL2Parts, 0.0), &sp->l2_part))) {
    tdnnf_supervision_destroy(sp);
    return rc;
  }
  if (tables) {
    const size_t parts = (size_t)B * ((T + kNumWideFrames - 1) / kNumWideFrames);
    hipError_t e = hipSuccess;
    if ((rc = to_device(pf_src, &sp->pf_src)) || (rc = to_device(pf_dst, &sp->pf_dst)) || (rc = to_device(pf_pdf, &sp->pf_pdf)) ||
        (rc = to_device(pf_t, &sp->pf_t)) || (rc = to_device(pf_lp, &sp->pf_lp)) ||
        (e = hipMalloc((void **)&sp->xent_part, sizeof(double) * parts)) != hipSuccess ||
        (sp->wide && ((e = hipMalloc((void **)&sp->la_own, sizeof(double) * (size_t)NS)) != hipSuccess ||
                      (e = hipMalloc((void **)&sp->lb_own, sizeof(double) * (size_t)NS)) != hipSuccess))) {
      tdnnf_supervision_destroy(sp);
      return rc ? rc : hip_status(e, "supervision_create: hipMalloc");
    }
  }
  *out = sp;
  return TDNNF_OK;
}

int tdnnf_supervision_info(const tdnnf_supervision *sp, int *num_states, int *num_arcs, int *max_states_per_frame, int *wide) {
  TDNNF_REQUIRE(sp, "supervision_info: null supervision");
  if (num_states) *num_states = sp->num_states;
  if (num_arcs) *num_arcs = sp->num_arcs;
  if (max_states_per_frame) *max_states_per_frame = sp->max_states_per_frame;
  if (wide) *wide = sp->wide ? 1 : 0;
  return TDNNF_OK;
}

void tdnnf_supervision_destroy(tdnnf_supervision *sp) {
  if (!sp) return;
  if (sp->ts) {  // reserved, time-synchronous: every device array is a piece of the one allocation (chain_sup_build.hip)
    sup_reserved_free(sp);
    delete sp;
    return;
  }
  void *ptrs[] = {sp->seq_state_begin, sp->state_time, sp->final_logprob, sp->in_begin, sp->in_src, sp->in_pdf,
                  sp->in_lp, sp->out_begin, sp->out_dst, sp->out_pdf, sp->out_lp, sp->frame_state_begin,
                  sp->la_own, sp->lb_own, sp->pf_src, sp->pf_dst, sp->pf_pdf, sp->pf_t, sp->pf_lp, sp->xent_part,
                  sp->e2e_alpha, sp->e2e_beta, sp->e2e_vecs, sp->l2_part};
  for (void *p : ptrs) hipFree(p);
  tdnnf_align_graphs_destroy(sp->e2e_graphs);  // (end-to-end kind: chain_num_e2e.hip; null otherwise)
  delete sp;
}

}  // extern "C"
