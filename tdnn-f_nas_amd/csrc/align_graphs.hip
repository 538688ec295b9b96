// align_graphs.hip -- creates, describes and destroys a tdnnf_align_graphs (include/tdnnf_hip.h, "best-path alignment"): validates the caller's
// arrays, builds the three arc tables (four for labelled graphs) on the host (align_tables.h) and uploads them.  Its readers: align.hip, align_fb.hip, align_sparse.hip, chain_num_e2e.hip.
#include <math.h>

#include "align_graphs.h"

namespace tdnnf {
namespace {

// a device copy of v (one element at least) as D, which has T's bytes
template <class D, class T>
int align_to_device(const std::vector<T> &v, const D **out) {
  static_assert(sizeof(D) == sizeof(T), "copied byte for byte");
  void *p = nullptr;
  TDNNF_HIP(hipMalloc(&p, sizeof(T) * std::max<size_t>(v.size(), 1)));
  *out = static_cast<const D *>(p);
  if (!v.empty()) TDNNF_HIP(hipMemcpy(p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
  return TDNNF_OK;
}

int align_table_to_device(const AlignHostTable &h, AlignTable *t) {
  int rc;
  if ((rc = align_to_device(h.slots, &t->slots)) || (rc = align_to_device(h.heavy, &t->heavy))) return rc;
  return align_to_device(h.arcs, &t->arcs);
}

// tdnnf_align_graphs_create (arc_label null) and tdnnf_align_graphs_create_labelled.  who: the prefix of the messages, the call's name.
int align_graphs_create(const char *who, int num_graphs, int num_pdfs, const int *graph_state_begin, const int *graph_arc_begin, const int *arc_src,
                        const int *arc_dst, const int *arc_pdf, const float *arc_logprob, const float *initial_logprob, const float *final_logprob,
                        const int *arc_label, int num_labels, tdnnf_align_graphs **out) {
  TDNNF_REQUIRE(out && num_graphs > 0 && num_pdfs > 0 && graph_state_begin && graph_arc_begin && arc_src && arc_dst && arc_pdf && arc_logprob &&
                    initial_logprob && final_logprob,
                "%sbad arguments", who);
  TDNNF_REQUIRE(graph_state_begin[0] == 0 && graph_arc_begin[0] == 0, "%sgraph_state_begin and graph_arc_begin must start at 0", who);
  const int NS = graph_state_begin[num_graphs];
  for (int g = 0; g < num_graphs; g++) {
    const int s0 = graph_state_begin[g], s1 = graph_state_begin[g + 1], a0 = graph_arc_begin[g], a1 = graph_arc_begin[g + 1];
    TDNNF_REQUIRE(s1 > s0 && a1 >= a0, "%sgraph %d must have at least one state and a non-negative arc count", who, g);
    bool has_init = false, has_final = false;
    for (int s = s0; s < s1; s++) {
      has_init = has_init || initial_logprob[s] > -INFINITY;
      has_final = has_final || final_logprob[s] > -INFINITY;
    }
    TDNNF_REQUIRE(has_init, "%sgraph %d has no initial state (no initial_logprob above -inf)", who, g);
    TDNNF_REQUIRE(has_final, "%sgraph %d has no final state (no final_logprob above -inf)", who, g);
    for (int a = a0; a < a1; a++) {
      TDNNF_REQUIRE(arc_src[a] >= s0 && arc_src[a] < s1 && arc_dst[a] >= s0 && arc_dst[a] < s1,
                    "%sarc %d (state %d -> %d) leaves graph %d's states [%d, %d)", who, a, arc_src[a], arc_dst[a], g, s0, s1);
      TDNNF_REQUIRE(arc_pdf[a] >= 0 && arc_pdf[a] < num_pdfs, "%sarc %d carries pdf %d outside [0, %d) (epsilon arcs are not supported)", who, a,
                    arc_pdf[a], num_pdfs);
      TDNNF_REQUIRE(!arc_label || (arc_label[a] >= 0 && arc_label[a] < num_labels), "%sarc %d carries label %d outside [0, %d)", who, a,
                    arc_label ? arc_label[a] : 0, num_labels);
    }
  }
  AlignHostTables t;
  align_build_tables(num_graphs, num_pdfs, graph_state_begin, graph_arc_begin, arc_src, arc_dst, arc_pdf, arc_logprob, &t, true, arc_label);
  TDNNF_REQUIRE(t.by_dst.arcs.size() < (size_t)1 << 31, "%sthe sliced arc table has more than 2^31 entries", who);
  TDNNF_REQUIRE(t.by_src.arcs.size() < (size_t)1 << 31 && t.by_pdf.arcs.size() < (size_t)1 << 31,
                "%sa sliced arc table (by source, by pdf) has more than 2^31 entries", who);
  TDNNF_REQUIRE(t.by_label.arcs.size() < (size_t)1 << 31, "%sthe sliced arc table by label has more than 2^31 entries", who);
  tdnnf_align_graphs *g = new tdnnf_align_graphs();
  g->G = num_graphs;
  g->P = num_pdfs;
  g->dev = AlignDev{};
  g->state_begin.assign(graph_state_begin, graph_state_begin + num_graphs + 1);
  for (int k = 0; k < num_graphs; k++) g->num_arcs.push_back(graph_arc_begin[k + 1] - graph_arc_begin[k]);
  g->max_in_degree = t.max_in_degree;
  g->col_begin = t.col_begin;
  g->col_pdfs = t.col_pdfs;
  g->num_cols_dev = nullptr;
  g->col_pdfs_dev = nullptr;
  g->L = arc_label ? num_labels : 0;
  g->lcol_begin = t.lcol_begin;
  g->col_labels = t.col_labels;
  g->by_label = AlignTable{};
  g->label_range_dev = nullptr;
  g->num_lcols_dev = g->col_labels_dev = g->arc_label_dev = nullptr;
  std::vector<int> num_cols;
  for (int k = 0; k < num_graphs; k++) num_cols.push_back(t.col_begin[k + 1] - t.col_begin[k]);
  const std::vector<float> init(initial_logprob, initial_logprob + NS), fin(final_logprob, final_logprob + NS);
  int rc;
  if ((rc = align_to_device(t.graphs, &g->dev.graphs)) || (rc = align_table_to_device(t.by_dst, &g->dev.by_dst)) ||
      (rc = align_table_to_device(t.by_src, &g->dev.by_src)) || (rc = align_table_to_device(t.by_pdf, &g->dev.by_pdf)) ||
      (rc = align_to_device(init, &g->dev.init)) || (rc = align_to_device(fin, &g->dev.final)) || (rc = align_to_device(num_cols, &g->num_cols_dev)) ||
      (rc = align_to_device(t.col_pdfs, &g->col_pdfs_dev))) {
    tdnnf_align_graphs_destroy(g);
    return rc;
  }
  if (arc_label) {
    std::vector<int> num_lcols;
    for (int k = 0; k < num_graphs; k++) num_lcols.push_back(t.lcol_begin[k + 1] - t.lcol_begin[k]);
    const std::vector<int> labels(arc_label, arc_label + graph_arc_begin[num_graphs]);
    if ((rc = align_table_to_device(t.by_label, &g->by_label)) || (rc = align_to_device(t.label_range, &g->label_range_dev)) ||
        (rc = align_to_device(num_lcols, &g->num_lcols_dev)) || (rc = align_to_device(t.col_labels, &g->col_labels_dev)) ||
        (rc = align_to_device(labels, &g->arc_label_dev))) {
      tdnnf_align_graphs_destroy(g);
      return rc;
    }
  }
  *out = g;
  return TDNNF_OK;
}

}  // namespace
}  // namespace tdnnf

using namespace tdnnf;

extern "C" {

int tdnnf_align_graphs_create(int num_graphs, int num_pdfs, const int *graph_state_begin, const int *graph_arc_begin, const int *arc_src,
                              const int *arc_dst, const int *arc_pdf, const float *arc_logprob, const float *initial_logprob,
                              const float *final_logprob, tdnnf_align_graphs **out) {
  return align_graphs_create("align_graphs_create: ", num_graphs, num_pdfs, graph_state_begin, graph_arc_begin, arc_src, arc_dst, arc_pdf, arc_logprob,
                             initial_logprob, final_logprob, nullptr, 0, out);
}

int tdnnf_align_graphs_create_labelled(int num_graphs, int num_pdfs, const int *graph_state_begin, const int *graph_arc_begin, const int *arc_src,
                                       const int *arc_dst, const int *arc_pdf, const float *arc_logprob, const float *initial_logprob,
                                       const float *final_logprob, const int *arc_label, int num_labels, tdnnf_align_graphs **out) {
  const char *who = "align_graphs_create_labelled: ";
  TDNNF_REQUIRE(arc_label && num_labels > 0, "%snull arc_label or num_labels %d", who, num_labels);
  return align_graphs_create(who, num_graphs, num_pdfs, graph_state_begin, graph_arc_begin, arc_src, arc_dst, arc_pdf, arc_logprob, initial_logprob,
                             final_logprob, arc_label, num_labels, out);
}

void tdnnf_align_graphs_destroy(tdnnf_align_graphs *g) {
  if (!g) return;
  const AlignDev &d = g->dev;
  const void *ptrs[] = {d.graphs,      d.by_dst.slots, d.by_dst.heavy, d.by_dst.arcs, d.by_src.slots, d.by_src.heavy,
                        d.by_src.arcs, d.by_pdf.slots, d.by_pdf.heavy, d.by_pdf.arcs, d.init,         d.final,
                        g->num_cols_dev, g->col_pdfs_dev, g->by_label.slots, g->by_label.heavy, g->by_label.arcs, g->label_range_dev,
                        g->num_lcols_dev, g->col_labels_dev, g->arc_label_dev};
  for (const void *p : ptrs) (void)hipFree(const_cast<void *>(p));
  delete g;
}

int tdnnf_align_graphs_info(const tdnnf_align_graphs *g, int graph, int *num_states, int *num_arcs, int *max_in_degree) {
  TDNNF_REQUIRE(g && graph >= 0 && graph < g->G, "align_graphs_info: null graphs or graph %d out of range", graph);
  if (num_states) *num_states = g->state_begin[graph + 1] - g->state_begin[graph];
  if (num_arcs) *num_arcs = g->num_arcs[graph];
  if (max_in_degree) *max_in_degree = g->max_in_degree[graph];
  return TDNNF_OK;
}

int tdnnf_align_graphs_pdfs(const tdnnf_align_graphs *g, int graph, int *num, int *pdfs_out) {
  TDNNF_REQUIRE(g && graph >= 0 && graph < g->G, "align_graphs_pdfs: null graphs or graph %d out of range", graph);
  const int c0 = g->col_begin[graph], c1 = g->col_begin[graph + 1];
  if (num) *num = c1 - c0;
  if (pdfs_out) std::copy(g->col_pdfs.begin() + c0, g->col_pdfs.begin() + c1, pdfs_out);
  return TDNNF_OK;
}

int tdnnf_align_graphs_labels(const tdnnf_align_graphs *g, int graph, int *num, int *labels_out) {
  int rc = align_need_labels(g, "align_graphs_labels: ");
  if (rc) return rc;
  TDNNF_REQUIRE(graph >= 0 && graph < g->G, "align_graphs_labels: graph %d out of range", graph);
  const int c0 = g->lcol_begin[graph], c1 = g->lcol_begin[graph + 1];
  if (num) *num = c1 - c0;
  if (labels_out) std::copy(g->col_labels.begin() + c0, g->col_labels.begin() + c1, labels_out);
  return TDNNF_OK;
}

}  // extern "C"
