// align_graphs.h -- the device copy of a set of pdf-labelled graphs (tdnnf_align_graphs), shared by its two readers: align.hip (best path;
// builds and reads the arcs by destination) and align_fb.hip (forward-backward; reads them too and adds the arcs by source and by pdf).
#pragma once
#include <vector>

#include "align_kernels.h"

namespace tdnnf {
namespace {

// One more grouping of a set's arcs, laid out as align.hip lays out the arcs by destination (align_kernels.h): the rows of at most
// kAlignHeavy arcs sorted by descending length and cut into slices of 64, the heavy rows one after the other; a row's arcs in the
// caller's order.  What a row is and what an arc's int4 holds is the table's own (align_fb_kernels.h).
struct AlignFbTable {
  const int4 *slots;  // (row LOCAL to its graph or -1 for an empty lane, length, position of the row's first arc: its j-th is 64 j further, 0)
  const int4 *heavy;  // (LOCAL row, first arc, one past the last arc, 0)
  const int4 *arcs;
};
struct AlignFbGraphDev {  // one graph's share of the two tables
  int src_slot0, src_num_slots, src_heavy0, src_num_heavy;
  int pdf_slot0, pdf_num_slots, pdf_heavy0, pdf_num_heavy;
};

}  // namespace
}  // namespace tdnnf

struct tdnnf_align_graphs {
  int G, P;
  std::vector<int> state_begin, num_arcs, max_in_degree;  // host: [G + 1], [G], [G]
  tdnnf::AlignGraphDev *graphs;
  int4 *slots, *heavy, *arcs;
  float *init, *final;
  // forward-backward (align_fb.hip): by source -- rows are states, every state has one; by pdf -- rows are the pdfs that an arc of the graph names
  tdnnf::AlignFbGraphDev *fb_graphs;
  int4 *src_slots, *src_heavy, *src_arcs;
  int4 *pdf_slots, *pdf_heavy, *pdf_arcs;
};

namespace tdnnf {
// (align_fb.hip; not part of the library's symbol table)  Fills the fb_* / src_* / pdf_* members from the arrays tdnnf_align_graphs_create
// has validated; align_fb_tables_free releases them (null members are fine).
__attribute__((visibility("hidden"))) int align_fb_tables_create(tdnnf_align_graphs *g, const int *graph_state_begin, const int *graph_arc_begin,
                                                                 const int *arc_src, const int *arc_dst, const int *arc_pdf, const float *arc_logprob);
__attribute__((visibility("hidden"))) void align_fb_tables_free(tdnnf_align_graphs *g);
}  // namespace tdnnf
