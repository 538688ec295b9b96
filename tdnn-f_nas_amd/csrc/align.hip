// align.hip -- best-path alignment (include/tdnnf_hip.h, "best-path alignment"): builds the device copy of a set of pdf-labelled graphs
// (arcs by destination: the light rows in slices of 64, the heavy rows one after the other), sizes and lays out the workspace, launches align_best_path_kernel (align_kernels.h).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "align_graphs.h"
#include "chain_plan.h"

namespace tdnnf {
namespace {

template <class T>
int align_to_device(const std::vector<T> &v, T **out) {
  *out = nullptr;
  TDNNF_HIP(hipMalloc((void **)out, sizeof(T) * std::max<size_t>(v.size(), 1)));
  if (!v.empty()) TDNNF_HIP(hipMemcpy(*out, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
  return TDNNF_OK;
}

inline size_t round_up(size_t n, size_t m) { return (n + m - 1) / m * m; }

// What a call runs as and where its arrays lie behind the (16-byte aligned) start of the workspace:
//   [AlignUtt x num_utts, padded to 256 bytes] [back-pointers: per utterance frames * S ints, padded to an even count]
//   [global form only: per utterance 2 * S doubles]
struct AlignPlan {
  int threads;  // 64 for graphs of at most 64 states, 256 up to 1024 states, 1024 above (the largest graph an utterance of the call names decides)
  bool lds;
  bool row_in_lds;  // LDS form with two output rows behind the vectors (align_kernels.h, YLDS)
  size_t lds_bytes;
  int max_states;
  size_t desc_bytes, bp_ints, vec_doubles, bytes;
  std::vector<AlignUtt> utts;
};

int align_graph_of(const tdnnf_align_graphs *g, int num_utts, const int *utt_graph, int u) {
  if (utt_graph) return utt_graph[u];
  return g->G == 1 ? 0 : u;
}

int align_plan(const tdnnf_align_graphs *g, int num_utts, const int *utt_graph, const int *utt_frames, const int *utt_row_begin, AlignPlan *p) {
  TDNNF_REQUIRE(g && num_utts > 0 && utt_frames, "align: null graphs, no utterances or null utt_frames");
  TDNNF_REQUIRE(utt_graph || g->G == 1 || g->G == num_utts, "align: utt_graph may be null only for one graph or one graph per utterance");
  p->utts.resize(num_utts);
  p->max_states = 0;
  size_t bp = 0, vec = 0;
  long long out = 0;
  for (int u = 0; u < num_utts; u++) {
    const int gi = align_graph_of(g, num_utts, utt_graph, u);
    TDNNF_REQUIRE(gi >= 0 && gi < g->G, "align: utterance %d names graph %d of %d", u, gi, g->G);
    TDNNF_REQUIRE(utt_frames[u] >= 0, "align: utterance %d has %d frames", u, utt_frames[u]);
    const int S = g->state_begin[gi + 1] - g->state_begin[gi];
    p->max_states = std::max(p->max_states, S);
    AlignUtt &d = p->utts[u];
    d.graph = gi;
    d.frames = utt_frames[u];
    d.row_begin = utt_row_begin ? utt_row_begin[u] : 0;
    d.out_begin = (int)out;
    d.bp_begin = (long long)bp;
    d.vec_begin = (long long)vec;
    out += utt_frames[u];
    TDNNF_REQUIRE(out + num_utts < (1ll << 31), "align: more than 2^31 frames in one call");
    bp += round_up((size_t)utt_frames[u] * (size_t)S, 2);
    vec += 2 * (size_t)S;
  }
  const bool fits = 2 * sizeof(double) * (size_t)p->max_states <= kLdsBudget;
  const int form = options().align_form;
  TDNNF_REQUIRE(form >= 0 && form <= 2, "align: option align_form must be 0, 1 or 2");
  TDNNF_REQUIRE(form != 1 || fits, "align: option align_form = 1, but two vectors of %d doubles do not fit the LDS", p->max_states);
  p->lds = form == 1 || (form == 0 && fits);
  p->threads = p->max_states <= 64 ? 64 : p->max_states <= 1024 ? 256 : 1024;
  const size_t vec_bytes = 2 * sizeof(double) * (size_t)p->max_states, rows_bytes = 2 * sizeof(float) * (size_t)g->P;
  p->row_in_lds = p->lds && g->P <= kAlignRowRegs * p->threads && vec_bytes + rows_bytes <= kLdsBudget;
  p->lds_bytes = p->lds ? vec_bytes + (p->row_in_lds ? rows_bytes : 0) : 0;
  p->desc_bytes = round_up(sizeof(AlignUtt) * (size_t)num_utts, 256);
  p->bp_ints = bp;
  p->vec_doubles = p->lds ? 0 : vec;
  p->bytes = 16 + p->desc_bytes + sizeof(int) * p->bp_ints + sizeof(double) * p->vec_doubles;
  return TDNNF_OK;
}

template <int NT, bool LDS, bool YLDS>
int align_launch_form(const AlignPlan &p, int P, const AlignDev &dev, const AlignUtt *utts, const MatView &y, int row_stride, float acoustic_scale, int *bp,
                      double *vecs, int *pdf_out, int *state_out, double *results, hipStream_t s) {
  if (LDS) TDNNF_HIP(hipFuncSetAttribute((const void *)align_best_path_kernel<NT, LDS, YLDS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes));
  hipLaunchKernelGGL((align_best_path_kernel<NT, LDS, YLDS>), dim3((int)p.utts.size()), dim3(NT), p.lds_bytes, s, dev, utts, y, row_stride, acoustic_scale,
                     bp, vecs, pdf_out, state_out, results, p.max_states, P);
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

template <int NT>
int align_launch(const AlignPlan &p, int P, const AlignDev &dev, const AlignUtt *utts, const MatView &y, int row_stride, float acoustic_scale, int *bp,
                 double *vecs, int *pdf_out, int *state_out, double *results, hipStream_t s) {
  if (p.row_in_lds) return align_launch_form<NT, true, true>(p, P, dev, utts, y, row_stride, acoustic_scale, bp, vecs, pdf_out, state_out, results, s);
  if (p.lds) return align_launch_form<NT, true, false>(p, P, dev, utts, y, row_stride, acoustic_scale, bp, vecs, pdf_out, state_out, results, s);
  return align_launch_form<NT, false, false>(p, P, dev, utts, y, row_stride, acoustic_scale, bp, vecs, pdf_out, state_out, results, s);
}

}  // namespace
}  // namespace tdnnf

using namespace tdnnf;

extern "C" {

int tdnnf_align_graphs_create(int num_graphs, int num_pdfs, const int *graph_state_begin, const int *graph_arc_begin, const int *arc_src,
                              const int *arc_dst, const int *arc_pdf, const float *arc_logprob, const float *initial_logprob,
                              const float *final_logprob, tdnnf_align_graphs **out) {
  TDNNF_REQUIRE(out && num_graphs > 0 && num_pdfs > 0 && graph_state_begin && graph_arc_begin && arc_src && arc_dst && arc_pdf && arc_logprob &&
                    initial_logprob && final_logprob,
                "align_graphs_create: bad arguments");
  TDNNF_REQUIRE(graph_state_begin[0] == 0 && graph_arc_begin[0] == 0, "align_graphs_create: graph_state_begin and graph_arc_begin must start at 0");
  const int NS = graph_state_begin[num_graphs], NA = graph_arc_begin[num_graphs];
  for (int g = 0; g < num_graphs; g++) {
    const int s0 = graph_state_begin[g], s1 = graph_state_begin[g + 1], a0 = graph_arc_begin[g], a1 = graph_arc_begin[g + 1];
    TDNNF_REQUIRE(s1 > s0 && a1 >= a0, "align_graphs_create: graph %d must have at least one state and a non-negative arc count", g);
    bool has_init = false, has_final = false;
    for (int s = s0; s < s1; s++) {
      has_init = has_init || initial_logprob[s] > -INFINITY;
      has_final = has_final || final_logprob[s] > -INFINITY;
    }
    TDNNF_REQUIRE(has_init, "align_graphs_create: graph %d has no initial state (no initial_logprob above -inf)", g);
    TDNNF_REQUIRE(has_final, "align_graphs_create: graph %d has no final state (no final_logprob above -inf)", g);
    for (int a = a0; a < a1; a++) {
      TDNNF_REQUIRE(arc_src[a] >= s0 && arc_src[a] < s1 && arc_dst[a] >= s0 && arc_dst[a] < s1,
                    "align_graphs_create: arc %d (state %d -> %d) leaves graph %d's states [%d, %d)", a, arc_src[a], arc_dst[a], g, s0, s1);
      TDNNF_REQUIRE(arc_pdf[a] >= 0 && arc_pdf[a] < num_pdfs, "align_graphs_create: arc %d carries pdf %d outside [0, %d) (epsilon arcs are not supported)", a,
                    arc_pdf[a], num_pdfs);
    }
  }
  std::vector<int> state_graph(NS);
  for (int g = 0; g < num_graphs; g++)
    for (int s = graph_state_begin[g]; s < graph_state_begin[g + 1]; s++) state_graph[s] = g;
  // per destination, the caller's arc order
  std::vector<std::vector<int>> in(NS);
  for (int a = 0; a < NA; a++) in[arc_dst[a]].push_back(a);
  auto packed = [&](int a) {
    int bits;
    memcpy(&bits, &arc_logprob[a], 4);
    return make_int4(arc_src[a] - graph_state_begin[state_graph[arc_src[a]]], arc_pdf[a], bits, a);
  };
  tdnnf_align_graphs *g = new tdnnf_align_graphs();
  g->G = num_graphs;
  g->P = num_pdfs;
  g->graphs = nullptr;
  g->slots = g->heavy = nullptr;
  g->arcs = nullptr;
  g->init = g->final = nullptr;
  g->fb_graphs = nullptr;
  g->src_slots = g->src_heavy = g->src_arcs = g->pdf_slots = g->pdf_heavy = g->pdf_arcs = nullptr;
  g->state_begin.assign(graph_state_begin, graph_state_begin + num_graphs + 1);
  std::vector<AlignGraphDev> gd(num_graphs);
  std::vector<int4> arcs, slots, heavy;
  for (int k = 0; k < num_graphs; k++) {
    const int s0 = graph_state_begin[k], s1 = graph_state_begin[k + 1];
    gd[k].state0 = s0;
    gd[k].num_states = s1 - s0;
    gd[k].slot0 = (int)slots.size();
    gd[k].heavy0 = (int)heavy.size();
    // light rows by descending in-degree (stable), so that the 64 rows of a slice have near-equal lengths
    std::vector<int> light;
    int deg = 0;
    for (int s = s0; s < s1; s++) {
      const int d = (int)in[s].size();
      deg = std::max(deg, d);
      if (d <= kAlignHeavy) light.push_back(s);
    }
    std::stable_sort(light.begin(), light.end(), [&](int a, int b) { return in[a].size() > in[b].size(); });
    for (size_t first = 0; first < light.size(); first += 64) {
      const size_t base = arcs.size(), width = in[light[first]].size();
      arcs.resize(base + 64 * width, make_int4(0, 0, 0, -1));  // (entries beyond a row's length are never read)
      for (int lane = 0; lane < 64; lane++) {
        if (first + lane >= light.size()) {
          slots.push_back(make_int4(-1, 0, 0, 0));
          continue;
        }
        const int s = light[first + lane];
        slots.push_back(make_int4(s - s0, (int)in[s].size(), (int)base + lane, 0));
        for (size_t j = 0; j < in[s].size(); j++) arcs[base + 64 * j + lane] = packed(in[s][j]);
      }
    }
    gd[k].num_slots = (int)slots.size() - gd[k].slot0;
    for (int s = s0; s < s1; s++) {
      if ((int)in[s].size() <= kAlignHeavy) continue;
      heavy.push_back(make_int4(s - s0, (int)arcs.size(), (int)(arcs.size() + in[s].size()), 0));
      for (int a : in[s]) arcs.push_back(packed(a));
    }
    gd[k].num_heavy = (int)heavy.size() - gd[k].heavy0;
    g->num_arcs.push_back(graph_arc_begin[k + 1] - graph_arc_begin[k]);
    g->max_in_degree.push_back(deg);
  }
  if (arcs.size() >= (size_t)1 << 31) {
    delete g;
    TDNNF_REQUIRE(false, "align_graphs_create: the sliced arc table has more than 2^31 entries");
  }
  std::vector<float> init(initial_logprob, initial_logprob + NS), fin(final_logprob, final_logprob + NS);
  int rc;
  if ((rc = align_to_device(gd, &g->graphs)) || (rc = align_to_device(slots, &g->slots)) || (rc = align_to_device(heavy, &g->heavy)) ||
      (rc = align_to_device(arcs, &g->arcs)) || (rc = align_to_device(init, &g->init)) || (rc = align_to_device(fin, &g->final)) ||
      (rc = align_fb_tables_create(g, graph_state_begin, graph_arc_begin, arc_src, arc_dst, arc_pdf, arc_logprob))) {
    tdnnf_align_graphs_destroy(g);
    return rc;
  }
  *out = g;
  return TDNNF_OK;
}

void tdnnf_align_graphs_destroy(tdnnf_align_graphs *g) {
  if (!g) return;
  void *ptrs[] = {g->graphs, g->slots, g->heavy, g->arcs, g->init, g->final};
  for (void *p : ptrs) hipFree(p);
  align_fb_tables_free(g);
  delete g;
}

int tdnnf_align_graphs_info(const tdnnf_align_graphs *g, int graph, int *num_states, int *num_arcs, int *max_in_degree) {
  TDNNF_REQUIRE(g && graph >= 0 && graph < g->G, "align_graphs_info: null graphs or graph %d out of range", graph);
  if (num_states) *num_states = g->state_begin[graph + 1] - g->state_begin[graph];
  if (num_arcs) *num_arcs = g->num_arcs[graph];
  if (max_in_degree) *max_in_degree = g->max_in_degree[graph];
  return TDNNF_OK;
}

size_t tdnnf_align_workspace_bytes(const tdnnf_align_graphs *g, int num_utts, const int *utt_graph, const int *utt_frames) {
  AlignPlan p;
  if (align_plan(g, num_utts, utt_graph, utt_frames, nullptr, &p) != TDNNF_OK) return 0;
  return p.bytes;
}

int tdnnf_align_best_path(const tdnnf_align_graphs *g, int num_utts, const int *utt_graph, const int *utt_frames, const int *utt_row_begin,
                          int row_stride, const tdnnf_mat *nnet_output, float acoustic_scale, int *pdf_out_dev, int *state_out_dev,
                          double *results_dev, void *workspace_dev, size_t workspace_bytes, tdnnf_stream stream) {
  TDNNF_REQUIRE(g && utt_row_begin && mat_ok(nnet_output) && pdf_out_dev && results_dev && workspace_dev, "align_best_path: bad arguments");
  TDNNF_REQUIRE(row_stride >= 1, "align_best_path: row_stride %d", row_stride);
  TDNNF_REQUIRE(nnet_output->cols >= g->P, "align_best_path: nnet_output has %d columns, the graphs %d pdfs", nnet_output->cols, g->P);
  AlignPlan p;
  int rc = align_plan(g, num_utts, utt_graph, utt_frames, utt_row_begin, &p);
  if (rc) return rc;
  for (int u = 0; u < num_utts; u++) {
    const long long last = (long long)utt_row_begin[u] + (long long)(utt_frames[u] - 1) * row_stride;
    TDNNF_REQUIRE(utt_row_begin[u] >= 0 && (utt_frames[u] == 0 || last < nnet_output->rows),
                  "align_best_path: utterance %d reads rows %d .. %lld of a matrix of %d rows", u, utt_row_begin[u], last, nnet_output->rows);
  }
  TDNNF_REQUIRE(workspace_bytes >= p.bytes, "align_best_path: workspace of %zu bytes, %zu needed (tdnnf_align_workspace_bytes)", workspace_bytes, p.bytes);
  hipStream_t s = (hipStream_t)stream;
  char *base = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(workspace_dev) + 15) & ~(uintptr_t)15);
  AlignUtt *utts = reinterpret_cast<AlignUtt *>(base);
  int *bp = reinterpret_cast<int *>(base + p.desc_bytes);
  double *vecs = reinterpret_cast<double *>(base + p.desc_bytes + sizeof(int) * p.bp_ints);
  // (pageable source: the runtime has taken the table by the time the call returns)
  TDNNF_HIP(hipMemcpyAsync(utts, p.utts.data(), sizeof(AlignUtt) * (size_t)num_utts, hipMemcpyHostToDevice, s));
  const AlignDev dev{g->graphs, g->slots, g->heavy, g->arcs, g->init, g->final};
  const MatView y = view(nnet_output);
  switch (p.threads) {
    case 64:
      return align_launch<64>(p, g->P, dev, utts, y, row_stride, acoustic_scale, bp, vecs, pdf_out_dev, state_out_dev, results_dev, s);
    case 256:
      return align_launch<256>(p, g->P, dev, utts, y, row_stride, acoustic_scale, bp, vecs, pdf_out_dev, state_out_dev, results_dev, s);
    default:
      return align_launch<1024>(p, g->P, dev, utts, y, row_stride, acoustic_scale, bp, vecs, pdf_out_dev, state_out_dev, results_dev, s);
  }
}

}  // extern "C"
