// align_graphs.hip -- creates, describes and destroys a tdnnf_align_graphs (include/tdnnf_hip.h, "best-path alignment"): validates the caller's
// arrays, builds the three arc tables on the host (align_tables.h) and uploads them.  Its readers: align.hip, align_fb.hip, align_sparse.hip, chain_num_e2e.hip.
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
  const int NS = graph_state_begin[num_graphs];
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
  AlignHostTables t;
  align_build_tables(num_graphs, num_pdfs, graph_state_begin, graph_arc_begin, arc_src, arc_dst, arc_pdf, arc_logprob, &t, true);
  TDNNF_REQUIRE(t.by_dst.arcs.size() < (size_t)1 << 31, "align_graphs_create: the sliced arc table has more than 2^31 entries");
  TDNNF_REQUIRE(t.by_src.arcs.size() < (size_t)1 << 31 && t.by_pdf.arcs.size() < (size_t)1 << 31,
                "align_graphs_create: a sliced arc table (by source, by pdf) has more than 2^31 entries");
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
  *out = g;
  return TDNNF_OK;
}

void tdnnf_align_graphs_destroy(tdnnf_align_graphs *g) {
  if (!g) return;
  const AlignDev &d = g->dev;
  const void *ptrs[] = {d.graphs,      d.by_dst.slots, d.by_dst.heavy, d.by_dst.arcs, d.by_src.slots, d.by_src.heavy,
                        d.by_src.arcs, d.by_pdf.slots, d.by_pdf.heavy, d.by_pdf.arcs, d.init,         d.final,
                        g->num_cols_dev, g->col_pdfs_dev};
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

}  // extern "C"
