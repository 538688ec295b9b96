// align_graphs.hip -- creates, describes and destroys a tdnnf_align_graphs (include/tdnnf_hip.h, "best-path alignment"): validates the caller's
// arrays, builds the three arc tables (four for labelled graphs) on the host (align_tables.h) and uploads them.  And the reusable kind:
// tdnnf_align_graphs_reserve allocates a handle once for a capacity, tdnnf_align_graphs_assign validates a batch, stages it and enqueues the
// copies and the device build (align_build.hip) on the caller's stream; tdnnf_align_graphs_assign_transcripts does the same from unit
// sequences (a tdnnf_unit_set; the host side in align_transcripts.h), with the compile kernel (align_compile.hip) writing the arc arrays in
// front of the build, and tdnnf_align_graphs_assign_pronunciations from transcripts whose positions have alternative unit sequences
// (align_pronunciations.h, align_pron_compile.hip); tdnnf_align_graphs_dump copies the device arrays of either kind out for tests.  Its readers: align.hip, align_fb.hip, align_sparse.hip, chain_num_e2e.hip.
#include <math.h>
#include <string.h>

#include <utility>

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

// What tdnnf_align_graphs_create and tdnnf_align_graphs_assign validate of the caller's arrays.  who: the prefix of the messages, the call's name.
int align_validate(const char *who, bool have_out, int num_graphs, int num_pdfs, const int *graph_state_begin, const int *graph_arc_begin, const int *arc_src,
                   const int *arc_dst, const int *arc_pdf, const float *arc_logprob, const float *initial_logprob, const float *final_logprob,
                   const int *arc_label, int num_labels) {
  TDNNF_REQUIRE(have_out && num_graphs > 0 && num_pdfs > 0 && graph_state_begin && graph_arc_begin && arc_src && arc_dst && arc_pdf && arc_logprob &&
                    initial_logprob && final_logprob,
                "%sbad arguments", who);
  TDNNF_REQUIRE(graph_state_begin[0] == 0 && graph_arc_begin[0] == 0, "%sgraph_state_begin and graph_arc_begin must start at 0", who);
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
  return TDNNF_OK;
}

// tdnnf_align_graphs_create (arc_label null) and tdnnf_align_graphs_create_labelled.  who: the prefix of the messages, the call's name.
int align_graphs_create(const char *who, int num_graphs, int num_pdfs, const int *graph_state_begin, const int *graph_arc_begin, const int *arc_src,
                        const int *arc_dst, const int *arc_pdf, const float *arc_logprob, const float *initial_logprob, const float *final_logprob,
                        const int *arc_label, int num_labels, tdnnf_align_graphs **out) {
  if (int rc = align_validate(who, out != nullptr, num_graphs, num_pdfs, graph_state_begin, graph_arc_begin, arc_src, arc_dst, arc_pdf, arc_logprob,
                              initial_logprob, final_logprob, arc_label, num_labels))
    return rc;
  const int NS = graph_state_begin[num_graphs];
  AlignHostTables t;
  align_build_tables(num_graphs, num_pdfs, graph_state_begin, graph_arc_begin, arc_src, arc_dst, arc_pdf, arc_logprob, &t, true, arc_label);
  TDNNF_REQUIRE(t.by_dst.arcs.size() < (size_t)1 << 31, "%sthe sliced arc table has more than 2^31 entries", who);
  TDNNF_REQUIRE(t.by_src.arcs.size() < (size_t)1 << 31 && t.by_pdf.arcs.size() < (size_t)1 << 31,
                "%sa sliced arc table (by source, by pdf) has more than 2^31 entries", who);
  TDNNF_REQUIRE(t.by_label.arcs.size() < (size_t)1 << 31, "%sthe sliced arc table by label has more than 2^31 entries", who);
  tdnnf_align_graphs *g = new tdnnf_align_graphs();
  g->G = num_graphs;
  g->P = num_pdfs;
  const AlignHostTable *tables[4] = {&t.by_dst, &t.by_src, &t.by_pdf, &t.by_label};
  for (int i = 0; i < 4; i++) {
    g->table_counts[i][0] = (long long)tables[i]->slots.size();
    g->table_counts[i][1] = (long long)tables[i]->heavy.size();
    g->table_counts[i][2] = (long long)tables[i]->arcs.size();
  }
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

// ---- reserved handles: one device allocation for the capacities, refilled in stream order by tdnnf_align_graphs_assign (assign_stage.h)

// the rows a table can have in a batch at the capacities: a state table's are the states; by_pdf's and by_label's the distinct pdfs / labels
// of each graph, at most its arcs and at most num_pdfs / num_labels a graph
long long align_row_capacity(const tdnnf_align_graphs *g, int table) {
  if (table < 2) return g->cap_states;
  return std::min<long long>(g->cap_arcs, (long long)g->cap_graphs * (table == 2 ? g->P : g->L));
}

// Every device array of a reserved handle, the build's scratch and the device staging, out of c.  Run once with a null base for the size.
void align_reserve_layout(tdnnf_align_graphs *g, Carve *c) {
  const size_t Gc = g->cap_graphs, Sc = g->cap_states, Ac = g->cap_arcs;
  AlignBuildDev &b = g->build;
  b.graphs = c->take<AlignGraphDev>(Gc);
  g->dev.graphs = b.graphs;
  g->dev.init = c->take<float>(Sc);
  g->dev.final = c->take<float>(Sc);
  g->num_cols_dev = c->take<int>(Gc);
  g->col_pdfs_dev = b.col_pdfs = c->take<int>(align_row_capacity(g, 2));
  b.num_tables = g->L > 0 ? 4 : 3;
  if (g->L > 0) {
    g->label_range_dev = b.label_range = c->take<AlignRange>(Gc);
    g->num_lcols_dev = c->take<int>(Gc);
    g->col_labels_dev = b.col_labels = c->take<int>(align_row_capacity(g, 3));
    g->arc_label_dev = b.label = c->take<int>(Ac);
  }
  AlignTable *tables[4] = {&g->dev.by_dst, &g->dev.by_src, &g->dev.by_pdf, &g->by_label};
  for (int i = 0; i < b.num_tables; i++) {
    const long long rows = align_row_capacity(g, i);
    const AlignTableBound bound = align_table_bound(g->cap_graphs, rows, g->cap_arcs);
    AlignBuildTable &t = b.t[i];
    t.cap_slots = (int)bound.slots;
    t.cap_heavy = (int)bound.heavy;
    t.cap_arcs = (int)bound.arcs;
    tables[i]->slots = t.slots = c->take<int4>(bound.slots);
    tables[i]->heavy = t.heavy = c->take<int4>(bound.heavy);
    tables[i]->arcs = t.arcs = c->take<int4>(bound.arcs);
    t.len = c->take<int>(rows);
    t.order = c->take<int>(rows);
    t.rowpos = c->take<int>(rows);
    t.off = c->take<int>(rows);
    t.arcpos = c->take<int>(Ac);
    t.ginfo = c->take<int4>(Gc);
    t.gbase = c->take<int4>(Gc);
    t.totals = c->take<int>(4);
  }
  g->stage.dev = c->take<char>(g->stage.bytes);
}

// What both assigns check under the call's name `who`, on either side of their own validation.  In front of it the handle: a reserved
// one, and reserved for labels exactly when the batch brings them (`labels`).  Behind it the batch's totals: the three capacities.
int align_assign_handle(const char *who, const tdnnf_align_graphs *g, bool labels) {
  TDNNF_REQUIRE(g->reserved, "%sthe handle was made by tdnnf_align_graphs_create: only a handle of tdnnf_align_graphs_reserve can be assigned", who);
  TDNNF_REQUIRE(g->L == 0 || labels, "%sthe handle was reserved for labels (num_labels %d), and arc_label is null", who, g->L);
  TDNNF_REQUIRE(g->L > 0 || !labels, "%sarc_label given to a handle that was reserved without labels (num_labels 0)", who);
  return TDNNF_OK;
}
int align_assign_fits(const char *who, const tdnnf_align_graphs *g, int G, int NS, int NA) {
  std::string err;
  TDNNF_REQUIRE(within_capacity(who, G, "graphs", g->cap_graphs, &err) && within_capacity(who, NS, "states", g->cap_states, &err) && within_capacity(who, NA, "arcs", g->cap_arcs, &err),
                "%s", err.c_str());
  return TDNNF_OK;
}

}  // namespace

int align_build_launch(const AlignBuildDev &b, int max_graph_arcs, int max_graph_rows, hipStream_t s);  // align_build.hip
int align_compile_launch(const AlignCompileDev &c, int G, hipStream_t s);                                // align_compile.hip

int align_pron_compile_launch(const AlignPronCompileDev &c, int G, hipStream_t s);                       // align_pron_compile.hip

// The end of every assign: the copies, the compile in front of the build (compile(): the transcript or pronunciation kernel's launch, or
// nothing) and the build on s, then the host metadata of the batch (p's, moved out of it).  From the first enqueued copy the device tables are
// being overwritten: the handle holds no batch until all of it succeeded (assign_stage.h).
template <class Compile>
static int align_commit(tdnnf_align_graphs *g, const StagePacker &pk, size_t raw_bytes, Compile compile, TranscriptPlan &&p, hipStream_t s) {
  const int assigns_before = g->assigns;
  g->assigns = 0;
  int rc;
  if ((rc = g->stage.submit(pk, raw_bytes, s)) || (rc = compile()) ||
      (rc = align_build_launch(g->build, p.max_graph_arcs, p.max_graph_rows, s)))
    return rc;
  g->G = g->build.G;
  g->state_begin = std::move(p.state_begin);
  g->num_arcs = std::move(p.num_arcs);
  g->max_in_degree = std::move(p.max_in_degree);
  g->col_begin = std::move(p.col_begin);
  g->col_pdfs = std::move(p.col_pdfs);
  g->lcol_begin = std::move(p.lcol_begin);
  g->col_labels = std::move(p.col_labels);
  g->assigns = assigns_before + 1;
  return TDNNF_OK;
}

}  // namespace tdnnf

using namespace tdnnf;

extern "C" {

int tdnnf_align_graphs_reserve(int max_graphs, int num_pdfs, int num_labels, int max_states, int max_arcs, tdnnf_align_graphs **out) {
  const char *who = "align_graphs_reserve: ";
  TDNNF_REQUIRE(out && max_graphs > 0 && num_pdfs > 0 && num_labels >= 0 && max_states > 0 && max_arcs >= 0,
                "%sbad arguments (max_graphs %d, num_pdfs %d, num_labels %d, max_states %d, max_arcs %d)", who, max_graphs, num_pdfs, num_labels, max_states,
                max_arcs);
  TDNNF_REQUIRE(max_states >= max_graphs, "%smax_states %d is below max_graphs %d: every graph has a state", who, max_states, max_graphs);
  const AlignTableBound most = align_table_bound(max_graphs, std::max(max_states, max_arcs), max_arcs);
  TDNNF_REQUIRE(most.arcs < 1ll << 31 && most.slots < 1ll << 31, "%sa sliced arc table at these capacities has more than 2^31 entries", who);
  tdnnf_align_graphs *g = new tdnnf_align_graphs();
  g->P = num_pdfs;
  g->L = num_labels;
  g->reserved = true;
  g->cap_graphs = max_graphs;
  g->cap_states = max_states;
  g->cap_arcs = max_arcs;
  // staging: four begin arrays, four arrays per arc and the labels, two per state, the two column lists and their lengths
  const size_t stage_bytes = sizeof(int) * (4 * ((size_t)max_graphs + 1) + 7 * (size_t)max_arcs + 2 * (size_t)max_states + 2 * (size_t)max_graphs);
  if (int rc = g->stage.create("align_graphs_reserve: allocation", stage_bytes, [g](Carve *c) { align_reserve_layout(g, c); })) {
    tdnnf_align_graphs_destroy(g);
    return rc;
  }
  *out = g;
  return TDNNF_OK;
}

int tdnnf_align_graphs_assign(tdnnf_align_graphs *g, int num_graphs, const int *graph_state_begin, const int *graph_arc_begin, const int *arc_src,
                              const int *arc_dst, const int *arc_pdf, const float *arc_logprob, const float *initial_logprob,
                              const float *final_logprob, const int *arc_label, tdnnf_stream stream) {
  const char *who = "align_graphs_assign: ";
  TDNNF_REQUIRE(g, "%snull graphs", who);
  int rc;
  if ((rc = align_assign_handle(who, g, arc_label != nullptr)) ||
      (rc = align_validate(who, true, num_graphs, g->P, graph_state_begin, graph_arc_begin, arc_src, arc_dst, arc_pdf, arc_logprob, initial_logprob,
                           final_logprob, arc_label, g->L)))
    return rc;
  const int G = num_graphs, NS = graph_state_begin[G], NA = graph_arc_begin[G];
  if ((rc = align_assign_fits(who, g, G, NS, NA))) return rc;

  // the metadata the host answers layout questions from: lengths, largest in-degree, the column lists (sort and unique over a graph's arcs)
  TranscriptPlan p;  // (what a transcript batch's plan holds of its graphs, align_transcripts.h: the same fields)
  p.state_begin.assign(graph_state_begin, graph_state_begin + G + 1);
  p.col_begin.assign(1, 0);
  p.lcol_begin.assign(1, 0);
  p.max_graph_arcs = p.max_graph_rows = 0;
  std::vector<int> in_degree(NS, 0), list;
  const auto columns = [&](const int *of_arc, int a0, int a1, std::vector<int> *begin, std::vector<int> *cols) {
    list.assign(of_arc + a0, of_arc + a1);
    return append_columns(&list, begin, cols);
  };
  for (int k = 0; k < G; k++) {
    const int a0 = graph_arc_begin[k], a1 = graph_arc_begin[k + 1];
    p.num_arcs.push_back(a1 - a0);
    for (int a = a0; a < a1; a++) in_degree[arc_dst[a]]++;
    p.max_in_degree.push_back(*std::max_element(in_degree.begin() + graph_state_begin[k], in_degree.begin() + graph_state_begin[k + 1]));
    p.num_cols.push_back(columns(arc_pdf, a0, a1, &p.col_begin, &p.col_pdfs));
    p.num_lcols.push_back(arc_label ? columns(arc_label, a0, a1, &p.lcol_begin, &p.col_labels) : 0);
    p.max_graph_arcs = std::max(p.max_graph_arcs, a1 - a0);
    p.max_graph_rows = std::max(p.max_graph_rows, std::max(graph_state_begin[k + 1] - graph_state_begin[k], std::max(p.num_cols[k], p.num_lcols[k])));
  }

  StagePacker pk;
  if ((rc = g->stage.begin(&pk))) return rc;
  AlignBuildDev &b = g->build;
  const auto raw = [&](const void *v, size_t n) { return reinterpret_cast<const int *>(g->stage.dev + pk.put(v, n)); };
  b.G = G;
  b.state_begin = raw(graph_state_begin, (size_t)G + 1);
  b.arc_begin = raw(graph_arc_begin, (size_t)G + 1);
  b.col_begin = raw(p.col_begin.data(), (size_t)G + 1);
  b.lcol_begin = raw(p.lcol_begin.data(), arc_label ? (size_t)G + 1 : 0);
  b.src = raw(arc_src, NA);
  b.dst = raw(arc_dst, NA);
  b.pdf = raw(arc_pdf, NA);
  b.lp_bits = raw(arc_logprob, NA);
  const size_t raw_bytes = pk.at;
  // the arrays that go to the handle's own device arrays as they are
  pk.put_to(g->dev.init, initial_logprob, NS);
  pk.put_to(g->dev.final, final_logprob, NS);
  pk.put_to(g->num_cols_dev, p.num_cols.data(), G);
  pk.put_to(g->col_pdfs_dev, p.col_pdfs.data(), p.col_pdfs.size());
  if (arc_label) {
    pk.put_to(g->arc_label_dev, arc_label, NA);
    pk.put_to(g->num_lcols_dev, p.num_lcols.data(), G);
    pk.put_to(g->col_labels_dev, p.col_labels.data(), p.col_labels.size());
  }
  TDNNF_REQUIRE(pk.fits(), "%sinternal: the batch needs %zu bytes of staging, the handle has %zu", who, pk.at, pk.size);
  return align_commit(g, pk, raw_bytes, [] { return TDNNF_OK; }, std::move(p), static_cast<hipStream_t>(stream));
}

// ---- transcript graphs: a unit set made once, and the assign that compiles a batch of transcripts on the device (align_transcripts.h,
// align_compile.hip)

int tdnnf_unit_set_create(int num_units, int num_pdfs, int context, const int *entry_pdf, const int *loop_pdf, const float *loop_logprob,
                          const float *leave_logprob, float take_logprob, float skip_logprob, tdnnf_unit_set **out) {
  const char *who = "unit_set_create: ";
  TDNNF_REQUIRE(out && num_units > 0 && num_units < 1 << 15 && num_pdfs > 0 && (context == 0 || context == 1) && entry_pdf && loop_pdf && loop_logprob &&
                    leave_logprob,
                "%sbad arguments (num_units %d of at most 32767, num_pdfs %d, context %d, or a null array)", who, num_units, num_pdfs, context);
  const size_t U = num_units, n = context ? (U + 1) * U : U;
  for (size_t i = 0; i < n; i++) {
    TDNNF_REQUIRE(entry_pdf[i] >= 0 && entry_pdf[i] < num_pdfs, "%sentry_pdf[%zu] is %d, outside [0, %d)", who, i, entry_pdf[i], num_pdfs);
    TDNNF_REQUIRE(loop_pdf[i] >= 0 && loop_pdf[i] < num_pdfs, "%sloop_pdf[%zu] is %d, outside [0, %d)", who, i, loop_pdf[i], num_pdfs);
  }
  tdnnf_unit_set *u = new tdnnf_unit_set();
  u->host.U = num_units;
  u->host.P = num_pdfs;
  u->host.context = context;
  u->host.entry_pdf.assign(entry_pdf, entry_pdf + n);
  u->host.loop_pdf.assign(loop_pdf, loop_pdf + n);
  u->host.loop_logprob.assign(loop_logprob, loop_logprob + U);
  u->host.leave_logprob.assign(leave_logprob, leave_logprob + U);
  u->host.take_logprob = take_logprob;
  u->host.skip_logprob = skip_logprob;
  u->arena = nullptr;
  const auto layout = [&](Carve c) {  // the four tables out of one allocation; with a null base only their size
    u->dev.entry_pdf = c.take<int>(n);
    u->dev.loop_pdf = c.take<int>(n);
    u->dev.loop_logprob = c.take<float>(U);
    u->dev.leave_logprob = c.take<float>(U);
    return c.at;
  };
  if (hipError_t e = hipMalloc(&u->arena, layout(Carve{nullptr, 0}))) {
    delete u;
    return hip_status(e, "unit_set_create: hipMalloc");
  }
  layout(Carve{static_cast<char *>(u->arena), 0});
  u->dev.take_logprob = take_logprob;
  u->dev.skip_logprob = skip_logprob;
  u->dev.U = num_units;
  u->dev.context = context;
  hipError_t e = hipMemcpy(const_cast<int *>(u->dev.entry_pdf), entry_pdf, sizeof(int) * n, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(const_cast<int *>(u->dev.loop_pdf), loop_pdf, sizeof(int) * n, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(const_cast<float *>(u->dev.loop_logprob), loop_logprob, sizeof(float) * U, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(const_cast<float *>(u->dev.leave_logprob), leave_logprob, sizeof(float) * U, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    tdnnf_unit_set_destroy(u);
    return hip_status(e, "unit_set_create: hipMemcpy");
  }
  *out = u;
  return TDNNF_OK;
}

void tdnnf_unit_set_destroy(tdnnf_unit_set *u) {
  if (!u) return;
  (void)hipFree(u->arena);
  delete u;
}

int tdnnf_transcript_graph_sizes(const tdnnf_unit_set *units, int num_transcripts, const int *slot_begin, const int *slot_unit, const int *slot_optional,
                                 int *states_out, int *arcs_out) {
  const char *who = "transcript_graph_sizes: ";
  TDNNF_REQUIRE(units, "%snull unit set", who);
  std::string err;
  TDNNF_REQUIRE(transcripts_validate(who, units->host, num_transcripts, slot_begin, slot_unit, slot_optional, &err), "%s", err.c_str());
  for (int k = 0; k < num_transcripts; k++) {
    int S, A;
    transcript_graph_size(units->host.context, slot_begin[k + 1] - slot_begin[k], slot_optional + slot_begin[k], &S, &A);
    if (states_out) states_out[k] = S;
    if (arcs_out) arcs_out[k] = A;
  }
  return TDNNF_OK;
}

int tdnnf_align_graphs_assign_transcripts(tdnnf_align_graphs *g, const tdnnf_unit_set *units, int num_transcripts, const int *slot_begin,
                                          const int *slot_unit, const int *slot_optional, tdnnf_stream stream) {
  const char *who = "align_graphs_assign_transcripts: ";
  TDNNF_REQUIRE(g && units, "%snull graphs or null unit set", who);
  const bool labelled = g->L > 0;  // (a transcript batch brings the labels the handle wants: an arc's is the slot of its destination)
  int rc;
  if ((rc = align_assign_handle(who, g, labelled))) return rc;
  TDNNF_REQUIRE(units->host.P == g->P, "%sthe unit set names %d pdfs, the handle was reserved for num_pdfs %d", who, units->host.P, g->P);
  std::string err;
  TDNNF_REQUIRE(transcripts_validate(who, units->host, num_transcripts, slot_begin, slot_unit, slot_optional, &err), "%s", err.c_str());
  TranscriptPlan p;
  TDNNF_REQUIRE(transcripts_plan(who, units->host, num_transcripts, slot_begin, slot_unit, slot_optional, labelled, &p, &err), "%s", err.c_str());
  const int G = num_transcripts, NS = p.state_begin[G], NA = p.arc_begin[G], N = slot_begin[G];
  TDNNF_REQUIRE(!labelled || p.max_slots <= g->L, "%sthe longest transcript has %d slots, and a slot is a label: the handle's num_labels = %d is short by %d", who,
                p.max_slots, g->L, p.max_slots - g->L);
  if ((rc = align_assign_fits(who, g, G, NS, NA))) return rc;

  StagePacker pk;
  if ((rc = g->stage.begin(&pk))) return rc;
  AlignBuildDev &b = g->build;
  AlignCompileDev c;
  const auto raw = [&](const int *v, size_t n) { return reinterpret_cast<const int *>(g->stage.dev + pk.put(v, n)); };
  b.G = G;
  b.state_begin = c.state_begin = raw(p.state_begin.data(), (size_t)G + 1);
  b.arc_begin = c.arc_begin = raw(p.arc_begin.data(), (size_t)G + 1);
  b.col_begin = raw(p.col_begin.data(), (size_t)G + 1);
  b.lcol_begin = raw(p.lcol_begin.data(), labelled ? (size_t)G + 1 : 0);
  c.slot_begin = raw(slot_begin, (size_t)G + 1);
  c.slots = raw(p.packed.data(), N);
  // the staging's two shapes: on the host the begins, the slots and the column lists; on the device the begins and the slots, behind them
  // the four arc arrays the kernel writes.  Both fit what tdnnf_align_graphs_reserve sized for 28 bytes an arc (slots < states, 2 <= arcs a graph)
  const size_t raw_bytes = pk.at, dev_bytes = raw_bytes + 4 * sizeof(int) * (size_t)NA;
  int *arcs = reinterpret_cast<int *>(g->stage.dev + raw_bytes);  // (device only)
  b.src = c.src = arcs;
  b.dst = c.dst = arcs + NA;
  b.pdf = c.pdf = arcs + 2 * (size_t)NA;
  b.lp_bits = c.lp_bits = arcs + 3 * (size_t)NA;
  c.label = labelled ? const_cast<int *>(g->arc_label_dev) : nullptr;
  c.init = const_cast<float *>(g->dev.init);
  c.final = const_cast<float *>(g->dev.final);
  c.units = units->dev;
  pk.put_to(g->num_cols_dev, p.num_cols.data(), p.num_cols.size());
  pk.put_to(g->col_pdfs_dev, p.col_pdfs.data(), p.col_pdfs.size());
  if (labelled) {
    pk.put_to(g->num_lcols_dev, p.num_lcols.data(), p.num_lcols.size());
    pk.put_to(g->col_labels_dev, p.col_labels.data(), p.col_labels.size());
  }
  TDNNF_REQUIRE(pk.fits() && dev_bytes <= pk.size, "%sinternal: the batch needs %zu bytes of staging on the host and %zu on the device, the handle has %zu", who,
                pk.at, dev_bytes, pk.size);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  return align_commit(g, pk, raw_bytes, [&] { return align_compile_launch(c, G, s); }, std::move(p), s);
}

// ---- pronunciation graphs: transcripts whose positions have alternatives (align_pronunciations.h, align_pron_compile.hip)

int tdnnf_pronunciation_graph_sizes(const tdnnf_unit_set *units, int num_transcripts, const int *pos_begin, const int *pos_optional, const int *pos_alt_begin,
                                    const float *alt_logprob, const int *alt_unit_begin, const int *alt_units, int *states_out, int *arcs_out) {
  const char *who = "pronunciation_graph_sizes: ";
  TDNNF_REQUIRE(units, "%snull unit set", who);
  const PronunciationBatch b = {num_transcripts, pos_begin, pos_optional, pos_alt_begin, alt_logprob, alt_unit_begin, alt_units};
  std::string err;
  TDNNF_REQUIRE(pronunciations_validate(who, units->host, b, &err), "%s", err.c_str());
  for (int k = 0; k < num_transcripts; k++) {
    const PronunciationSize z = pronunciation_graph_size(units->host.context, pos_begin[k + 1] - pos_begin[k], pos_optional + pos_begin[k],
                                                         pos_alt_begin + pos_begin[k], alt_unit_begin);
    TDNNF_REQUIRE(z.states < 1ll << 31 && z.arcs < 1ll << 31, "%stranscript %d has more than 2^31 states or arcs", who, k);
    if (states_out) states_out[k] = (int)z.states;
    if (arcs_out) arcs_out[k] = (int)z.arcs;
  }
  return TDNNF_OK;
}

int tdnnf_align_graphs_assign_pronunciations(tdnnf_align_graphs *g, const tdnnf_unit_set *units, int num_transcripts, const int *pos_begin,
                                             const int *pos_optional, const int *pos_alt_begin, const float *alt_logprob, const int *alt_unit_begin,
                                             const int *alt_units, tdnnf_stream stream) {
  const char *who = "align_graphs_assign_pronunciations: ";
  TDNNF_REQUIRE(g && units, "%snull graphs or null unit set", who);
  const bool labelled = g->L > 0;  // (the batch brings the labels the handle wants: an arc's is the entry of its destination)
  int rc;
  if ((rc = align_assign_handle(who, g, labelled))) return rc;
  TDNNF_REQUIRE(units->host.P == g->P, "%sthe unit set names %d pdfs, the handle was reserved for num_pdfs %d", who, units->host.P, g->P);
  const PronunciationBatch batch = {num_transcripts, pos_begin, pos_optional, pos_alt_begin, alt_logprob, alt_unit_begin, alt_units};
  std::string err;
  TDNNF_REQUIRE(pronunciations_validate(who, units->host, batch, &err), "%s", err.c_str());
  PronunciationPlan p;
  TDNNF_REQUIRE(pronunciations_plan(who, units->host, batch, labelled, &p, &err), "%s", err.c_str());
  const int G = num_transcripts, NS = p.state_begin[G], NA = p.arc_begin[G];
  const int NP = pos_begin[G], NQ = pos_alt_begin[NP], NE = alt_unit_begin[NQ];
  TDNNF_REQUIRE(!labelled || p.max_entries <= g->L,
                "%sthe largest transcript has %d entries (units of its alternatives), and an entry is a label: the handle's num_labels = %d is short by %d", who,
                p.max_entries, g->L, p.max_entries - g->L);
  if ((rc = align_assign_fits(who, g, G, NS, NA))) return rc;

  StagePacker pk;
  if ((rc = g->stage.begin(&pk))) return rc;
  AlignBuildDev &b = g->build;
  AlignPronCompileDev c;
  const auto raw = [&](const void *v, size_t n) { return reinterpret_cast<const int *>(g->stage.dev + pk.put(v, n)); };
  b.G = G;
  b.state_begin = c.state_begin = raw(p.state_begin.data(), (size_t)G + 1);
  b.arc_begin = c.arc_begin = raw(p.arc_begin.data(), (size_t)G + 1);
  b.col_begin = raw(p.col_begin.data(), (size_t)G + 1);
  b.lcol_begin = raw(p.lcol_begin.data(), labelled ? (size_t)G + 1 : 0);
  c.pos_begin = raw(pos_begin, (size_t)G + 1);
  c.pos_alt_begin = raw(pos_alt_begin, (size_t)NP + 1);
  c.pos_info = raw(p.pos_info.data(), NP);
  c.alt_unit_begin = raw(alt_unit_begin, (size_t)NQ + 1);
  c.alt_pos = raw(p.alt_pos.data(), NQ);
  c.alt_logprob = reinterpret_cast<const float *>(raw(alt_logprob, NQ));
  c.alt_units = raw(alt_units, NE);
  // The staging's two shapes, as the transcript assign's: on the host the tables above and the column lists; on the device the tables, behind
  // them the four arc arrays the kernel writes.  Both fit what tdnnf_align_graphs_reserve sized (28 bytes an arc, 8 a state, 24 a graph and
  // 16): the tables are at most pronunciations_raw_ints = 5 G + 7 + 2 positions + 3 alternatives + entries ints with positions <=
  // alternatives <= entries; every entry has a state beside the start (states >= G + entries), every entry has its loop and every first
  // entry's state an arc that enters it (arcs >= entries + alternatives).  So 3 arcs + 2 states + G >= 5 entries + 3 alternatives + 3 G
  // covers the tables behind the begins on the device, where 4 ints an arc follow; on the host the column lists are at most arcs + entries
  // ints and the four arc arrays are absent.  The check below refuses by name what this does not cover.
  const size_t raw_bytes = pk.at, dev_bytes = raw_bytes + 4 * sizeof(int) * (size_t)NA;
  int *arcs = reinterpret_cast<int *>(g->stage.dev + raw_bytes);  // (device only)
  b.src = c.src = arcs;
  b.dst = c.dst = arcs + NA;
  b.pdf = c.pdf = arcs + 2 * (size_t)NA;
  b.lp_bits = c.lp_bits = arcs + 3 * (size_t)NA;
  c.label = labelled ? const_cast<int *>(g->arc_label_dev) : nullptr;
  c.init = const_cast<float *>(g->dev.init);
  c.final = const_cast<float *>(g->dev.final);
  c.units = units->dev;
  pk.put_to(g->num_cols_dev, p.num_cols.data(), p.num_cols.size());
  pk.put_to(g->col_pdfs_dev, p.col_pdfs.data(), p.col_pdfs.size());
  if (labelled) {
    pk.put_to(g->num_lcols_dev, p.num_lcols.data(), p.num_lcols.size());
    pk.put_to(g->col_labels_dev, p.col_labels.data(), p.col_labels.size());
  }
  TDNNF_REQUIRE(pk.fits() && dev_bytes <= pk.size,
                "%sthe batch needs %zu bytes of staging on the host and %zu on the device, the handle's staging for max_states = %d and max_arcs = %d has %zu", who, pk.at,
                dev_bytes, g->cap_states, g->cap_arcs, pk.size);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  return align_commit(g, pk, raw_bytes, [&] { return align_pron_compile_launch(c, G, s); }, std::move(p), s);
}

int tdnnf_align_graphs_capacity(const tdnnf_align_graphs *g, int *max_graphs, int *max_states, int *max_arcs, long long *device_bytes, int *device_allocs,
                                int *assigns) {
  TDNNF_REQUIRE(g && g->reserved, "align_graphs_capacity: null graphs, or a handle that tdnnf_align_graphs_create made (it has no capacity)");
  if (max_graphs) *max_graphs = g->cap_graphs;
  if (max_states) *max_states = g->cap_states;
  if (max_arcs) *max_arcs = g->cap_arcs;
  if (device_bytes) *device_bytes = (long long)g->stage.arena_bytes;
  if (device_allocs) *device_allocs = g->stage.device_allocs;
  if (assigns) *assigns = g->assigns;
  return TDNNF_OK;
}

int tdnnf_align_graphs_dump(const tdnnf_align_graphs *g, int table, int which, int *out, long long capacity, long long *count) {
  const char *who = "align_graphs_dump: ";
  TDNNF_REQUIRE(g && count, "%snull graphs or null count", who);
  if (int rc = align_need_batch(g, who)) return rc;
  TDNNF_REQUIRE(table >= 0 && table <= 4 && which >= 0 && which <= (table < 4 ? 2 : 6), "%stable %d, which %d", who, table, which);
  TDNNF_REQUIRE(table != 3 || g->L > 0, "%sthe graphs carry no labels: there is no table 3", who);
  if (g->reserved) TDNNF_HIP(hipStreamSynchronize(g->stage.last_stream));
  const int NS = g->state_begin[g->G];
  long long NA = 0;
  for (int n : g->num_arcs) NA += n;
  // the pieces of the answer: (device array, ints)
  std::vector<std::pair<const void *, long long>> parts;
  if (table < 4) {
    const AlignTable &t = table == 0 ? g->dev.by_dst : table == 1 ? g->dev.by_src : table == 2 ? g->dev.by_pdf : g->by_label;
    long long entries = g->table_counts[table][which];
    if (g->reserved) {
      int totals[4];
      TDNNF_HIP(hipMemcpy(totals, g->build.t[table].totals, sizeof(totals), hipMemcpyDeviceToHost));
      entries = totals[which];
    }
    parts.push_back({which == 0 ? t.slots : which == 1 ? t.heavy : t.arcs, 4 * entries});
  } else if (which == 0) {
    parts.push_back({g->dev.graphs, (long long)(sizeof(AlignGraphDev) / sizeof(int)) * g->G});
  } else if (which == 1) {
    if (g->L > 0) parts.push_back({g->label_range_dev, (long long)(sizeof(AlignRange) / sizeof(int)) * g->G});
  } else if (which == 2) {
    parts.push_back({g->num_cols_dev, g->G});
    parts.push_back({g->col_pdfs_dev, (long long)g->col_pdfs.size()});
  } else if (which == 3) {
    if (g->L > 0) parts.push_back({g->num_lcols_dev, g->G});
    if (g->L > 0) parts.push_back({g->col_labels_dev, (long long)g->col_labels.size()});
  } else if (which == 4) {
    parts.push_back({g->dev.init, NS});
  } else if (which == 5) {
    parts.push_back({g->dev.final, NS});
  } else if (g->L > 0) {
    parts.push_back({g->arc_label_dev, NA});
  }
  long long total = 0;
  for (const auto &p : parts) total += p.second;
  *count = total;
  if (!out) return TDNNF_OK;
  TDNNF_REQUIRE(capacity >= total, "%sout holds %lld ints, the answer has %lld", who, capacity, total);
  for (const auto &p : parts) {
    if (p.second) TDNNF_HIP(hipMemcpy(out, p.first, sizeof(int) * (size_t)p.second, hipMemcpyDeviceToHost));
    out += p.second;
  }
  return TDNNF_OK;
}

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
  if (g->reserved) {  // every device array is a piece of the one allocation
    g->stage.destroy();
    delete g;
    return;
  }
  const AlignDev &d = g->dev;
  const void *ptrs[] = {d.graphs,      d.by_dst.slots, d.by_dst.heavy, d.by_dst.arcs, d.by_src.slots, d.by_src.heavy,
                        d.by_src.arcs, d.by_pdf.slots, d.by_pdf.heavy, d.by_pdf.arcs, d.init,         d.final,
                        g->num_cols_dev, g->col_pdfs_dev, g->by_label.slots, g->by_label.heavy, g->by_label.arcs, g->label_range_dev,
                        g->num_lcols_dev, g->col_labels_dev, g->arc_label_dev};
  for (const void *p : ptrs) (void)hipFree(const_cast<void *>(p));
  delete g;
}

int tdnnf_align_graphs_info(const tdnnf_align_graphs *g, int graph, int *num_states, int *num_arcs, int *max_in_degree) {
  if (int rc = align_need_batch(g, "align_graphs_info: ")) return rc;
  TDNNF_REQUIRE(g && graph >= 0 && graph < g->G, "align_graphs_info: null graphs or graph %d out of range", graph);
  if (num_states) *num_states = g->state_begin[graph + 1] - g->state_begin[graph];
  if (num_arcs) *num_arcs = g->num_arcs[graph];
  if (max_in_degree) *max_in_degree = g->max_in_degree[graph];
  return TDNNF_OK;
}

int tdnnf_align_graphs_pdfs(const tdnnf_align_graphs *g, int graph, int *num, int *pdfs_out) {
  if (int rc = align_need_batch(g, "align_graphs_pdfs: ")) return rc;
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
