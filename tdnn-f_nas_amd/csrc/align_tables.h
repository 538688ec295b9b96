// align_tables.h -- host side of a tdnnf_align_graphs, free of HIP (g++ compiles it: tests/test_align_tables_cpu.py, as host_linalg.h): the
// three arc tables of a set of pdf-labelled graphs (four when the caller labels the arcs) and the launch form of the recursions that walk them.
// align_graphs.hip uploads the tables; align.hip, align_fb.hip and chain_num_e2e.hip ask align_form_plan; the kernels (align_kernels.h, align_fb_kernels.h,
// num_e2e_kernels.h) read the tables through AlignDev (align_graphs.h).
//
// A table groups a set's arcs into ROWS, 16 bytes an arc: one load per arc.  The rows of at most kAlignHeavy arcs (light rows) are sorted by
// descending length (stable) and cut into SLICES of 64, one lane each: the j-th arcs of a slice's 64 rows lie side by side, so a wave's
// load of them is one contiguous KB (a thread per row over a CSR array touched 64 lines for the same KB: with batched loads 46 -> 24 us per
// frame on the 4 000-state graph, docs/experiments.md r6-o).  Unlike the denominator's SELL-64 tables, whose sums may take a row's arcs in
// any order, a row's arcs stay in the caller's order (j ascending), which is what the best path's tie rule and the sums' one order of
// summation need; a row is walked to its own length, so the padding of a slice is never read.  HEAVY rows (the denominator graph of a real
// system has states with hundreds of incoming arcs; a slice would pad 63 rows to that length) lie one after the other behind the slices
// and are taken a wave per row.
//   by_dst: rows are states (every state has one, empty or not); arc = (source state, pdf, log-prob bits, caller's arc index)
//   by_src: rows are states (likewise);                           arc = (destination state, pdf, log-prob bits, caller's arc index)
//   by_pdf: rows are the pdfs that an arc of the graph names;     arc = (source state, destination state, log-prob bits, caller's arc index)
//   by_label (labelled graphs only): rows are the labels that an arc of the graph carries, row r the r-th of them ascending; arc = (source state, destination state, log-prob bits, pdf)
//             -- the pdf where by_pdf has the caller's arc index, because a label's arcs name different pdfs.
// States are LOCAL to their graph everywhere.
// The pdfs that a graph's arcs name, ascending, are its COLUMN LIST (AlignHostTables::col_pdfs): a by_pdf row carries the rank of its pdf in
// that list -- its column -- in the 4th int of its slot or heavy-row descriptor, where the other two tables have 0.  The compact posteriors
// (align_fb_kernels.h) are addressed by it; the lists themselves stay on the host.  The labels of a graph's arcs, ascending, are its LABEL
// COLUMN LIST (col_labels) in the same way: a by_label row carries the rank of its label, and the label posteriors are addressed by it.
#pragma once
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

namespace tdnnf {

constexpr int kAlignHeavy = 64;       // a row of more arcs than this is a heavy row
constexpr int kAlignRowRegs = 8;      // floats of an output row a thread carries from one frame to the next (row_in_lds)
constexpr int kAlignFbAlphaRegs = 7;  // doubles of alpha_t a thread carries into LDS (alpha_in_lds): 7 * 1024 covers every S whose three vectors fit

struct AlignInt4 {  // the 16 bytes of a device int4
  int x, y, z, w;
};
static_assert(sizeof(AlignInt4) == 16, "copied into int4 arrays");

struct AlignRange {       // one graph's share of a table
  int slot0, num_slots;   // its light rows: slots[slot0 .. slot0 + num_slots), a multiple of 64
  int heavy0, num_heavy;  // its heavy rows: heavy[heavy0 .. heavy0 + num_heavy)
};
struct AlignGraphDev {     // one graph of a tdnnf_align_graphs (device table)
  int state0, num_states;  // its states are [state0, state0 + num_states) of the per-state arrays
  AlignRange by_dst, by_src, by_pdf;
};

struct AlignHostTable {
  std::vector<AlignInt4> slots;  // (row or -1 for an empty lane, length, position of the row's first arc: its j-th is 64 j further, column or 0)
  std::vector<AlignInt4> heavy;  // (row, first arc, one past the last arc, column or 0)
  std::vector<AlignInt4> arcs;
};

// One graph's rows into a table: rows[r] lists the arcs of row r in the caller's order; an empty row gets a slot of length 0 unless skip_empty.
// row_col (may be null: 0): what the 4th int of row r's slot or heavy-row descriptor carries.
template <class Pack>
AlignRange align_add_graph(AlignHostTable &t, const std::vector<std::vector<int>> &rows, bool skip_empty, const int *row_col, Pack packed) {
  AlignRange g;
  g.slot0 = (int)t.slots.size();
  g.heavy0 = (int)t.heavy.size();
  std::vector<int> light;
  for (int r = 0; r < (int)rows.size(); r++)
    if ((int)rows[r].size() <= kAlignHeavy && !(skip_empty && rows[r].empty())) light.push_back(r);
  std::stable_sort(light.begin(), light.end(), [&](int a, int b) { return rows[a].size() > rows[b].size(); });
  for (size_t first = 0; first < light.size(); first += 64) {
    const size_t base = t.arcs.size(), width = rows[light[first]].size();
    t.arcs.resize(base + 64 * width, AlignInt4{0, 0, 0, -1});  // (entries beyond a row's length are never read)
    for (int lane = 0; lane < 64; lane++) {
      if (first + lane >= light.size()) {
        t.slots.push_back(AlignInt4{-1, 0, 0, 0});
        continue;
      }
      const int r = light[first + lane];
      t.slots.push_back(AlignInt4{r, (int)rows[r].size(), (int)base + lane, row_col ? row_col[r] : 0});
      for (size_t j = 0; j < rows[r].size(); j++) t.arcs[base + 64 * j + lane] = packed(rows[r][j]);
    }
  }
  g.num_slots = (int)t.slots.size() - g.slot0;
  for (int r = 0; r < (int)rows.size(); r++) {
    if ((int)rows[r].size() <= kAlignHeavy) continue;
    t.heavy.push_back(AlignInt4{r, (int)t.arcs.size(), (int)(t.arcs.size() + rows[r].size()), row_col ? row_col[r] : 0});
    for (int a : rows[r]) t.arcs.push_back(packed(a));
  }
  g.num_heavy = (int)t.heavy.size() - g.heavy0;
  return g;
}

// Upper bounds on the three counts of ONE table that holds at most max_graphs graphs with total_rows rows and total_arcs arcs between them
// (a state table's rows are the states; by_pdf's and by_label's are the distinct pdfs / labels of each graph, never more than its arcs).
// A reserved tdnnf_align_graphs (align_graphs.hip) allocates its tables at these.  Per graph:
//   slots   a multiple of 64 that covers its light rows: at most roundup64(rows) <= rows + 63.
//   heavy   a heavy row has at least kAlignHeavy + 1 arcs and is a row: at most min(rows, arcs / 65).
//   arcs    its arcs and the padding of its slices.  The light rows are sorted by descending length, so in slice i, of width w_i (its first
//           row's length), lane 0 pads nothing and each of the 63 other lanes holds a row at least as long as the next slice's first, w_i+1:
//           the slice pads at most 63 (w_i - w_i+1).  The last slice, whose other lanes may be empty, pads at most 63 w_last.  The sum
//           telescopes to 63 w_0 <= 63 * kAlignHeavy = 4032 entries; a row of 64 arcs beside 63 empty rows (or alone) attains it.
struct AlignTableBound {
  long long slots, heavy, arcs;
};
constexpr int kAlignPadPerGraph = 63 * kAlignHeavy;
inline AlignTableBound align_table_bound(long long max_graphs, long long total_rows, long long total_arcs) {
  AlignTableBound b;
  b.slots = total_rows + 63 * max_graphs;
  b.heavy = std::min(total_rows, total_arcs / (kAlignHeavy + 1));
  b.arcs = total_arcs + (long long)kAlignPadPerGraph * max_graphs;
  return b;
}

struct AlignHostTables {
  std::vector<AlignGraphDev> graphs;
  AlignHostTable by_dst, by_src, by_pdf;
  std::vector<int> max_in_degree;  // per graph: the longest row by destination
  std::vector<int> col_begin;      // [graphs + 1]: graph k's column list is col_pdfs[col_begin[k] .. col_begin[k + 1])
  std::vector<int> col_pdfs;       // the distinct pdfs of a graph's arcs, ascending
  // labelled graphs only (align_build_tables with arc_label); AlignGraphDev does not grow, so the by_label ranges lie beside it
  AlignHostTable by_label;
  std::vector<AlignRange> label_range;  // [graphs]: graph k's share of by_label
  std::vector<int> lcol_begin;          // [graphs + 1]: graph k's label column list is col_labels[lcol_begin[k] .. lcol_begin[k + 1])
  std::vector<int> col_labels;          // the distinct labels of a graph's arcs, ascending
};

// The three tables of a set of graphs whose arrays tdnnf_align_graphs_create has validated (global state numbers, as the caller gives them),
// and the graphs' column lists.  columns: the by_pdf rows carry their columns, as tdnnf_align_graphs_create uploads them; without, the 4th
// int of every slot and descriptor is 0 (the tables as they were before there were columns, which tests/test_align_tables_cpu.py decodes).
// arc_label (may be null: no fourth table), one int per arc: the by_label table, whose rows always carry their columns, and
// the label column lists; the other three tables are what they are without labels.
inline void align_build_tables(int num_graphs, int num_pdfs, const int *graph_state_begin, const int *graph_arc_begin, const int *arc_src,
                               const int *arc_dst, const int *arc_pdf, const float *arc_logprob, AlignHostTables *t, bool columns = false,
                               const int *arc_label = nullptr) {
  t->graphs.resize(num_graphs);
  t->col_begin.assign(1, 0);
  t->lcol_begin.assign(1, 0);
  std::vector<int> col(num_pdfs);
  for (int k = 0; k < num_graphs; k++) {
    const int s0 = graph_state_begin[k], S = graph_state_begin[k + 1] - s0;
    std::vector<std::vector<int>> in(S), out(S), of_pdf(num_pdfs);
    for (int a = graph_arc_begin[k]; a < graph_arc_begin[k + 1]; a++) {
      in[arc_dst[a] - s0].push_back(a);
      out[arc_src[a] - s0].push_back(a);
      of_pdf[arc_pdf[a]].push_back(a);
    }
    auto bits = [&](int a) {
      int b;
      memcpy(&b, &arc_logprob[a], 4);
      return b;
    };
    AlignGraphDev &g = t->graphs[k];
    g.state0 = s0;
    g.num_states = S;
    for (int p = 0; p < num_pdfs; p++) {
      col[p] = (int)t->col_pdfs.size() - t->col_begin[k];  // (read for the pdfs with a row only)
      if (!of_pdf[p].empty()) t->col_pdfs.push_back(p);
    }
    t->col_begin.push_back((int)t->col_pdfs.size());
    g.by_dst = align_add_graph(t->by_dst, in, false, nullptr, [&](int a) { return AlignInt4{arc_src[a] - s0, arc_pdf[a], bits(a), a}; });
    g.by_src = align_add_graph(t->by_src, out, false, nullptr, [&](int a) { return AlignInt4{arc_dst[a] - s0, arc_pdf[a], bits(a), a}; });
    g.by_pdf = align_add_graph(t->by_pdf, of_pdf, true, columns ? col.data() : nullptr, [&](int a) { return AlignInt4{arc_src[a] - s0, arc_dst[a] - s0, bits(a), a}; });
    if (arc_label) {
      // (rows by rank, not by label: with the arc's own index as its label num_labels is the arcs of ALL graphs, and a row per label
      // per graph would be quadratic in the graphs)
      std::vector<int> list(arc_label + graph_arc_begin[k], arc_label + graph_arc_begin[k + 1]);
      std::sort(list.begin(), list.end());
      list.erase(std::unique(list.begin(), list.end()), list.end());
      std::vector<std::vector<int>> of_label(list.size());
      std::vector<int> rank(list.size());
      for (size_t r = 0; r < list.size(); r++) rank[r] = (int)r;
      for (int a = graph_arc_begin[k]; a < graph_arc_begin[k + 1]; a++)
        of_label[std::lower_bound(list.begin(), list.end(), arc_label[a]) - list.begin()].push_back(a);
      t->col_labels.insert(t->col_labels.end(), list.begin(), list.end());
      t->lcol_begin.push_back((int)t->col_labels.size());
      t->label_range.push_back(
          align_add_graph(t->by_label, of_label, true, rank.data(), [&](int a) { return AlignInt4{arc_src[a] - s0, arc_dst[a] - s0, bits(a), arc_pdf[a]}; }));
    }
    size_t deg = 0;
    for (const std::vector<int> &row : in) deg = std::max(deg, row.size());
    t->max_in_degree.push_back((int)deg);
  }
}

// What a recursion over graphs of at most max_states states and num_pdfs pdfs runs as: one workgroup per utterance.
struct AlignFormPlan {
  int threads;        // 64 for graphs of at most 64 states, 256 up to 1024 states, 1024 above
  bool lds;           // the two alternating state vectors in LDS (else in the caller's workspace / scratch)
  bool alpha_in_lds;  // a third vector behind them: alpha_t of the frame whose posteriors are formed (align_fb_kernels.h, ALDS)
  bool row_in_lds;    // behind the vectors two output rows of num_pdfs floats, staged one frame ahead (align_kernels.h, AlignRowStage)
  size_t lds_bytes;   // dynamic LDS of the launch
};

// align_form (option): 0 the vectors in LDS where two of them fit lds_budget, 1 / 2 force LDS / workspace.  want_alpha: the caller forms
// posteriors inside the recursion's kernel and would stage alpha_t.  False and *err (starting with prefix) for a form that cannot be had.
inline bool align_form_plan(int max_states, int num_pdfs, int align_form, bool want_alpha, size_t lds_budget, const char *prefix, AlignFormPlan *p,
                            std::string *err) {
  const size_t S8 = sizeof(double) * (size_t)max_states, rows_bytes = 2 * sizeof(float) * (size_t)num_pdfs;
  const bool fits = 2 * S8 <= lds_budget;
  char msg[200];
  if (align_form < 0 || align_form > 2) {
    snprintf(msg, sizeof(msg), "%soption align_form must be 0, 1 or 2", prefix);
    *err = msg;
    return false;
  }
  if (align_form == 1 && !fits) {
    snprintf(msg, sizeof(msg), "%soption align_form = 1, but two vectors of %d doubles do not fit the LDS", prefix, max_states);
    *err = msg;
    return false;
  }
  p->lds = align_form == 1 || (align_form == 0 && fits);
  p->threads = max_states <= 64 ? 64 : max_states <= 1024 ? 256 : 1024;
  p->alpha_in_lds = want_alpha && p->lds && 3 * S8 <= lds_budget && max_states <= kAlignFbAlphaRegs * p->threads;
  const size_t vec_bytes = (p->alpha_in_lds ? 3 : 2) * S8;
  // (with posteriors the rows are staged only behind a staged alpha_t: one launch form fewer, and a graph whose third vector does not fit has
  // little room left for rows)
  p->row_in_lds = p->lds && (!want_alpha || p->alpha_in_lds) && num_pdfs <= kAlignRowRegs * p->threads && vec_bytes + rows_bytes <= lds_budget;
  p->lds_bytes = p->lds ? vec_bytes + (p->row_in_lds ? rows_bytes : 0) : 0;
  return true;
}

// The interval of a checkpointing option (align_checkpoint, align_path_checkpoint: `name`) of value `value`: 0 off, C >= 1 the interval, -1
// automatic -- the least C with C * C >= max_frames, the call's longest utterance: ceil(sqrt(max_frames)).  An interval is at most that
// utterance (a longer one cuts no utterance differently) and at least 1.  False and *err (starting with prefix) for any other value.
inline bool align_checkpoint_interval(const char *name, int value, int max_frames, const char *prefix, int *C, std::string *err) {
  if (value < -1) {
    char msg[200];
    snprintf(msg, sizeof(msg), "%soption %s must be 0 (off), an interval >= 1 or -1 (automatic), not %d", prefix, name, value);
    *err = msg;
    return false;
  }
  const int longest = std::max(max_frames, 1);
  long long c = value;
  if (value == -1)
    for (c = 1; c * c < longest; c++) {
    }
  *C = (int)std::min<long long>(c, longest);
  return true;
}

// Alpha checkpointing of the forward-backward pass (option align_checkpoint; align_fb_kernels.h, CKPT).  With an interval C >= 1 an utterance
// of T frames is cut into the SEGMENTS [kC, min(kC + C, T)), k = 0 .. ceil(T / C) - 1; its alpha region holds, in this order,
//   the CHECKPOINTS   alpha_kC, one per segment (alpha_0 alone for T = 0: the forward pass always writes it), then
//   the SEGMENT BUFFER of min(C, T) - 1 vectors: slot j is alpha_(kC + 1 + j) of the segment k the backward pass is walking.
// alpha_T has no place: no frame's posteriors read it.  C = 0: alpha of every frame, T + 1 vectors, vector t is alpha_t.
struct AlignCheckpointPlan {
  int C;  // 0: off; else the interval, at most the call's longest utterance (a longer one cuts no utterance differently) and at least 1
  size_t checkpoints(int T) const { return C == 0 ? (size_t)T + 1 : T > 0 ? ((size_t)T - 1) / C + 1 : 1; }  // (C > 0: the segments of T >= 1 frames)
  size_t buffer(int T) const { return C == 0 || T < 1 ? 0 : (size_t)std::min(C, T) - 1; }
  size_t vectors(int T) const { return checkpoints(T) + buffer(T); }  // V(T, C), never more than T + 1
  int segments(int T) const { return C == 0 || T < 1 ? 0 : (T - 1) / C + 1; }
  int segment_begin(int k) const { return k * C; }
  int segment_end(int T, int k) const { return k * C + std::min(C, T - k * C); }
};

// align_checkpoint (option): 0 off, C >= 1 the interval, -1 automatic: the least C with C * C >= max_frames, the call's longest utterance --
// ceil(sqrt(max_frames)) -- and at least 1.  False and *err (starting with prefix) for any other value.
inline bool align_checkpoint_plan(int align_checkpoint, int max_frames, const char *prefix, AlignCheckpointPlan *p, std::string *err) {
  return align_checkpoint_interval("align_checkpoint", align_checkpoint, max_frames, prefix, &p->C, err);
}

// Back-pointer checkpointing of the best path (option align_path_checkpoint; align_kernels.h align_best_path_ckpt_kernel).  With an interval
// C >= 1 an utterance of T frames on a graph of S states is cut into the segments of AlignCheckpointPlan; its region of the workspace holds,
// in this order,
//   the CHECKPOINTS    alpha_kC, one vector of S doubles per segment (none for T = 0), written by the forward pass;
//   the SEGMENT BUFFER of min(C, T) frames of S back-pointers: frame j is the back-pointers of frame kC + j of the segment k that was last
//                      swept -- after the forward pass the last segment's, then those of the segment the trace-back has recomputed;
//   the PATH           T ints, the arc chosen for frame t (what option 0 leaves at bp[t * S]).
// Buffer and path are padded to an even count of ints each, so every region starts on 8 bytes.  C = 0: off, T * S back-pointers (align_call).
// align_kernels.h (align_path_regions) derives the same three offsets on the device from AlignUtt::frame_begin, T, S and C.
struct AlignPathCheckpointPlan {
  int C;  // 0: off; else the interval, at most the call's longest utterance and at least 1
  int segments(int T) const { return C == 0 || T < 1 ? 0 : (T - 1) / C + 1; }
  size_t checkpoints(int T) const { return (size_t)segments(T); }
  size_t buffer_frames(int T) const { return C == 0 ? (size_t)T : (size_t)std::min(C, T); }
  int segment_begin(int k) const { return k * C; }
  int segment_end(int T, int k) const { return k * C + std::min(C, T - k * C); }
  // the utterance's region in ints (4 bytes): 2 per double of a checkpoint
  size_t ints(int T, int S) const {
    if (C == 0) return ((size_t)T * (size_t)S + 1) / 2 * 2;
    return 2 * checkpoints(T) * (size_t)S + (buffer_frames(T) * (size_t)S + 1) / 2 * 2 + ((size_t)T + 1) / 2 * 2;
  }
};

// align_path_checkpoint (option): the values of align_checkpoint.  False and *err (starting with prefix) for any other value.
inline bool align_path_checkpoint_plan(int align_path_checkpoint, int max_frames, const char *prefix, AlignPathCheckpointPlan *p, std::string *err) {
  return align_checkpoint_interval("align_path_checkpoint", align_path_checkpoint, max_frames, prefix, &p->C, err);
}

}  // namespace tdnnf
