// align_graphs.h -- the device copy of a set of pdf-labelled graphs (tdnnf_align_graphs) and what its three readers share on the host:
// align.hip (best path), align_fb.hip (forward-backward), align_sparse.hip (its sparse output) and chain_num_e2e.hip (the end-to-end numerator).  align_graphs.hip creates and
// destroys the handle from the tables of align_tables.h, or reserves it once and has align_build.hip build the tables of each assigned batch on
// the device; the kernels take its AlignDev by value.
#pragma once
#include <string>
#include <vector>

#include "align_pronunciations.h"
#include "align_tables.h"
#include "align_transcripts.h"
#include "assign_stage.h"
#include "common.h"

namespace tdnnf {

struct AlignTable {   // one grouping of a set's arcs (align_tables.h), on the device
  const int4 *slots;  // (row LOCAL to its graph or -1 for an empty lane, length, position of the row's first arc: its j-th is 64 j further,
                      // by_pdf and by_label: the row's column, else 0)
  const int4 *heavy;  // (LOCAL row, first arc, one past the last arc, by_pdf and by_label: the row's column, else 0)
  const int4 *arcs;   // a row's arcs in the caller's order
};

struct AlignDev {
  const AlignGraphDev *graphs;
  AlignTable by_dst;          // rows: states; arcs (source state, pdf, log-prob bits, caller's arc index)
  AlignTable by_src;          // rows: states; arcs (destination state, pdf, log-prob bits, caller's arc index)
  AlignTable by_pdf;          // rows: pdfs;   arcs (source state, destination state, log-prob bits, caller's arc index)
  const float *init, *final;  // [total states]
};

struct AlignUtt {  // one utterance of a call (device table at the head of the workspace)
  int graph, frames;
  int row_begin;
  int out_begin;          // best path: first element of pdf_out; state_out starts at out_begin + (index of the utterance).  Forward-backward: 0,
                          // compact posteriors: first float of the utterance's block
  long long frame_begin;  // first element of its per-frame region of the workspace: best path -- the back-pointers, frames * S ints padded to an
                          // even count, or under option align_path_checkpoint the checkpoints, the segment buffer and the path
                          // (AlignPathCheckpointPlan; align.hip align_plan lays it out, still counted in ints); forward-backward -- alpha of every frame, (frames + 1) * S doubles (posteriors), or under option
                          // align_checkpoint the checkpoints and the segment buffer (AlignCheckpointPlan; align_fb.hip fb_plan lays it out)
  long long vec_begin;    // first double of its two state vectors in the workspace's vector region (workspace form)
};

static_assert(sizeof(AlignUtt) == 32, "the workspace formula of include/tdnnf_hip.h counts 32 bytes an utterance");

// ---- the device build of a reserved handle (align_build.hip, align_build_kernels.h): what its three kernels take by value
struct AlignBuildTable {  // one table as the build writes it, with its scratch
  int4 *slots, *heavy, *arcs;
  int cap_slots, cap_heavy, cap_arcs;  // the allocation's bounds (align_table_bound): no store goes beyond them
  int *len;     // [row capacity] arcs of a row; graph k's rows start at its row base (by_dst / by_src: its first state; by_pdf / by_label:
                // its first column), row r of by_pdf / by_label is the r-th entry of its column list
  int *order;   // [row capacity] per graph: its light rows by descending length (stable), behind them its heavy rows in row order
  int *rowpos;  // [row capacity] where a row stands in `order`
  int *off;     // [row capacity] per graph, local to its share of `arcs`: the first entry of each slice, behind them of each heavy row
  int *arcpos;  // [arc capacity] an arc's place in its row: the number of earlier arcs of its graph in the same row
  int4 *ginfo;  // [graph capacity] (slots, heavy rows, arc entries, light rows) of a graph
  int4 *gbase;  // [graph capacity] (first slot, first heavy row, first arc entry, 0) of a graph
  int *totals;  // [4] slots, heavy rows, arc entries of the batch
};
struct AlignBuildDev {
  // the batch's raw arrays (device staging)
  const int *state_begin, *arc_begin, *col_begin, *lcol_begin;  // [G + 1]
  const int *src, *dst, *pdf, *lp_bits, *label;                 // [arcs]; label null for an unlabelled handle
  const int *col_pdfs, *col_labels;                             // the column lists (the handle's own arrays)
  AlignBuildTable t[4];
  AlignGraphDev *graphs;    // [graph capacity]
  AlignRange *label_range;  // [graph capacity], labelled handles
  int G, num_tables;        // 3, or 4 with labels
};

// ---- the transcript compile of a reserved handle (align_compile.hip, align_compile_kernels.h): what its kernel takes by value
struct AlignUnitDev {  // a unit set's tables on the device (align_transcripts.h TranscriptUnits)
  const int *entry_pdf, *loop_pdf;
  const float *loop_logprob, *leave_logprob;
  float take_logprob, skip_logprob;
  int U, context;
};
struct AlignCompileDev {
  const int *slot_begin;               // [G + 1] (device staging)
  const int *slots;                    // per slot 2 * unit + optional (device staging)
  const int *state_begin, *arc_begin;  // [G + 1] (device staging)
  int *src, *dst, *pdf, *lp_bits;      // [arcs] device staging: what AlignBuildDev reads
  int *label;                          // [arcs] the handle's arc labels; null for an unlabelled handle
  float *init, *final;                 // [states] the handle's
  AlignUnitDev units;
};

// ---- the pronunciation compile of a reserved handle (align_pron_compile.hip, align_pron_compile_kernels.h): what its kernel takes by value
struct AlignPronCompileDev {
  const int *pos_begin;                // [G + 1] a transcript's positions (all tables: device staging)
  const int *pos_alt_begin;            // [positions + 1] a position's alternatives
  const int *pos_info;                 // [positions] 2 * (the position's first state, local to its graph) + optional
  const int *alt_unit_begin;           // [alternatives + 1] an alternative's entries
  const int *alt_pos;                  // [alternatives] its position
  const float *alt_logprob;            // [alternatives]
  const int *alt_units;                // [entries]
  const int *state_begin, *arc_begin;  // [G + 1]
  int *src, *dst, *pdf, *lp_bits;      // [arcs] device staging: what AlignBuildDev reads
  int *label;                          // [arcs] the handle's arc labels; null for an unlabelled handle
  float *init, *final;                 // [states] the handle's
  AlignUnitDev units;
};

}  // namespace tdnnf

struct tdnnf_unit_set {
  tdnnf::TranscriptUnits host;  // the tables as the caller gave them: validation, sizes and the column lists are host work
  tdnnf::AlignUnitDev dev;      // the same on the device, pieces of `arena`
  void *arena;                  // device, owned: the one allocation
};

struct tdnnf_align_graphs {
  int G, P;
  std::vector<int> state_begin, num_arcs, max_in_degree;  // host: [G + 1], [G], [G]
  tdnnf::AlignDev dev;                                    // device arrays, owned
  std::vector<int> col_begin, col_pdfs;                   // host: graph k's column list (align_tables.h) is col_pdfs[col_begin[k] .. col_begin[k + 1])
  const int *num_cols_dev;                                // device, owned: [G] the lengths of the column lists (the compact posteriors' row widths)
  const int *col_pdfs_dev;                                // device, owned: col_pdfs (the sparse posteriors' selection names a kept column's pdf)
  // labelled graphs (tdnnf_align_graphs_create_labelled) only; L = 0 and null pointers otherwise
  int L;                                     // num_labels
  std::vector<int> lcol_begin, col_labels;   // host: graph k's label column list (align_tables.h) is col_labels[lcol_begin[k] .. lcol_begin[k + 1])
  tdnnf::AlignTable by_label;                // device, owned: rows: labels; arcs (source state, destination state, log-prob bits, pdf).  Beside
                                             // AlignDev, which every kernel takes by value: the kernels without labels are what they were
  const tdnnf::AlignRange *label_range_dev;  // device, owned: [G] the graphs' shares of by_label (beside AlignGraphDev, which does not grow)
  const int *num_lcols_dev;                  // device, owned: [G] the lengths of the label column lists
  const int *col_labels_dev;                 // device, owned: col_labels
  const int *arc_label_dev;                  // device, owned: [arcs] the caller's labels in the caller's arc order (the labelled best path)
  // what tdnnf_align_graphs_dump copies out: [table 0 by_dst, 1 by_src, 2 by_pdf, 3 by_label][slots, heavy, arcs] entries.  A created handle's
  // are set at creation; a reserved handle's follow each assign on the device (AlignBuildDev::totals)
  long long table_counts[4][3];
  // ---- a RESERVED handle (tdnnf_align_graphs_reserve): every device array above is a piece of ONE allocation made for the capacities, the
  // pointers never change, and tdnnf_align_graphs_assign refills them in stream order (align_build.hip).  All zero for a created handle.
  bool reserved;
  int assigns;                           // assigns that succeeded; 0: no graphs (none yet, or an assign failed behind its first enqueued copy)
  int cap_graphs, cap_states, cap_arcs;  // the capacities: graphs, total states, total arcs of a batch
  tdnnf::AssignStage stage;              // the one allocation, the staging of the assigns, the allocation counts (assign_stage.h)
  tdnnf::AlignBuildDev build;            // the tables as the build kernels write them, and the build's scratch
};

namespace tdnnf {

// The refusal every entry gives a reserved handle that was never assigned a batch.  who: the prefix of the message, the call's name.
inline int align_need_batch(const tdnnf_align_graphs *g, const char *who) {
  TDNNF_REQUIRE(!g || !g->reserved || g->assigns > 0,
                "%sthe reserved graph set holds no graphs yet (tdnnf_align_graphs_assign gives it a batch)", who);
  return TDNNF_OK;
}

// The refusal every label entry gives a handle that tdnnf_align_graphs_create made.  who: the prefix of the message, the call's name.
inline int align_need_labels(const tdnnf_align_graphs *g, const char *who) {
  TDNNF_REQUIRE(g, "%snull graphs", who);
  if (int rc = align_need_batch(g, who)) return rc;
  TDNNF_REQUIRE(g->L > 0, "%sthe graphs carry no labels (tdnnf_align_graphs_create_labelled makes the handle this call takes)", who);
  return TDNNF_OK;
}

inline size_t align_round_up(size_t n, size_t m) { return (n + m - 1) / m * m; }

// The utterances of one call, for tdnnf_align_best_path (best_path) and tdnnf_align_posteriors and their *_workspace_bytes.
struct AlignCall {
  std::vector<AlignUtt> utts;
  int max_states;        // the largest graph an utterance of the call names
  size_t frame_elems;    // the per-frame regions together (ints or doubles: AlignUtt::frame_begin)
  size_t vec_doubles;    // the vector regions together: 2 * S doubles an utterance
  size_t desc_bytes;     // AlignUtt x num_utts, padded to 256 bytes
};

// Checks and describes the utterances.  plan / call: the prefixes of the messages ("align: " and "align_best_path: ").  nnet_output (may be
// null: the workspace question, no rows are named yet) and post_out (may be null) bound the rows an utterance reads and writes.
inline int align_call(const tdnnf_align_graphs *g, bool best_path, const char *plan, const char *call, int num_utts, const int *utt_graph,
                      const int *utt_frames, const int *utt_row_begin, int row_stride, const tdnnf_mat *nnet_output, const tdnnf_mat *post_out,
                      AlignCall *c) {
  TDNNF_REQUIRE(g && num_utts > 0 && utt_frames, "%snull graphs, no utterances or null utt_frames", plan);
  if (int rc = align_need_batch(g, plan)) return rc;
  TDNNF_REQUIRE(utt_graph || g->G == 1 || g->G == num_utts, "%sutt_graph may be null only for one graph or one graph per utterance", plan);
  c->utts.resize(num_utts);
  c->max_states = 0;
  size_t per_frame = 0, vec = 0;
  long long rows = 0;
  for (int u = 0; u < num_utts; u++) {
    const int gi = utt_graph ? utt_graph[u] : g->G == 1 ? 0 : u;
    TDNNF_REQUIRE(gi >= 0 && gi < g->G, "%sutterance %d names graph %d of %d", plan, u, gi, g->G);
    TDNNF_REQUIRE(utt_frames[u] >= 0, "%sutterance %d has %d frames", plan, u, utt_frames[u]);
    const int S = g->state_begin[gi + 1] - g->state_begin[gi];
    c->max_states = std::max(c->max_states, S);
    AlignUtt &d = c->utts[u];
    d.graph = gi;
    d.frames = utt_frames[u];
    d.row_begin = utt_row_begin ? utt_row_begin[u] : 0;
    d.out_begin = best_path ? (int)rows : 0;
    d.frame_begin = (long long)per_frame;
    d.vec_begin = (long long)vec;
    rows += utt_frames[u];
    TDNNF_REQUIRE(rows + num_utts < (1ll << 31), "%smore than 2^31 frames in one call", plan);
    per_frame += best_path ? align_round_up((size_t)utt_frames[u] * (size_t)S, 2) : ((size_t)utt_frames[u] + 1) * (size_t)S;
    vec += 2 * (size_t)S;
    if (!nnet_output) continue;
    const long long last = (long long)d.row_begin + (long long)(utt_frames[u] - 1) * row_stride;
    TDNNF_REQUIRE(d.row_begin >= 0 && (utt_frames[u] == 0 || last < nnet_output->rows), "%sutterance %d reads rows %d .. %lld of a matrix of %d rows",
                  call, u, d.row_begin, last, nnet_output->rows);
    TDNNF_REQUIRE(!post_out || utt_frames[u] == 0 || last < post_out->rows, "%sutterance %d writes rows %d .. %lld of a post_out of %d rows", call, u,
                  d.row_begin, last, post_out ? post_out->rows : 0);
  }
  c->frame_elems = per_frame;
  c->vec_doubles = vec;
  c->desc_bytes = align_round_up(sizeof(AlignUtt) * (size_t)num_utts, 256);
  return TDNNF_OK;
}

}  // namespace tdnnf
