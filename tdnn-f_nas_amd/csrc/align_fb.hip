// align_fb.hip -- forward-backward over pdf-labelled graphs (include/tdnnf_hip.h, "forward-backward"): adds the arcs by source and by pdf to a
// tdnnf_align_graphs at its creation (align.hip calls align_fb_tables_create), sizes and lays out the workspace, launches align_fb_kernel
// (align_fb_kernels.h).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "align_fb_kernels.h"
#include "chain_plan.h"

namespace tdnnf {
namespace {

template <class T>
int fb_to_device(const std::vector<T> &v, T **out) {
  *out = nullptr;
  TDNNF_HIP(hipMalloc((void **)out, sizeof(T) * std::max<size_t>(v.size(), 1)));
  if (!v.empty()) TDNNF_HIP(hipMemcpy(*out, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
  return TDNNF_OK;
}

inline size_t round_up(size_t n, size_t m) { return (n + m - 1) / m * m; }

struct FbHostTable {
  std::vector<int4> slots, heavy, arcs;
};

// One graph's rows into a table, as align.hip lays out a graph's arcs by destination: rows[r] lists the arcs of local row r in the caller's
// order; an empty row gets a slot of length 0 unless skip_empty.  The graph's slots / heavy rows are [*slot0, *slot0 + *num_slots) and
// [*heavy0, *heavy0 + *num_heavy).
template <class Pack>
void fb_add_graph(FbHostTable &t, const std::vector<std::vector<int>> &rows, bool skip_empty, Pack packed, int *slot0, int *num_slots, int *heavy0,
                  int *num_heavy) {
  *slot0 = (int)t.slots.size();
  *heavy0 = (int)t.heavy.size();
  std::vector<int> light;
  for (int r = 0; r < (int)rows.size(); r++)
    if ((int)rows[r].size() <= kAlignHeavy && !(skip_empty && rows[r].empty())) light.push_back(r);
  std::stable_sort(light.begin(), light.end(), [&](int a, int b) { return rows[a].size() > rows[b].size(); });
  for (size_t first = 0; first < light.size(); first += 64) {
    const size_t base = t.arcs.size(), width = rows[light[first]].size();
    t.arcs.resize(base + 64 * width, make_int4(0, 0, 0, -1));  // (entries beyond a row's length are never read)
    for (int lane = 0; lane < 64; lane++) {
      if (first + lane >= light.size()) {
        t.slots.push_back(make_int4(-1, 0, 0, 0));
        continue;
      }
      const int r = light[first + lane];
      t.slots.push_back(make_int4(r, (int)rows[r].size(), (int)base + lane, 0));
      for (size_t j = 0; j < rows[r].size(); j++) t.arcs[base + 64 * j + lane] = packed(rows[r][j]);
    }
  }
  *num_slots = (int)t.slots.size() - *slot0;
  for (int r = 0; r < (int)rows.size(); r++) {
    if ((int)rows[r].size() <= kAlignHeavy) continue;
    t.heavy.push_back(make_int4(r, (int)t.arcs.size(), (int)(t.arcs.size() + rows[r].size()), 0));
    for (int a : rows[r]) t.arcs.push_back(packed(a));
  }
  *num_heavy = (int)t.heavy.size() - *heavy0;
}

// What a call runs as and where its arrays lie behind the (16-byte aligned) start of the workspace:
//   [AlignFbUtt x num_utts, padded to 256 bytes] [posteriors: per utterance (frames + 1) * S doubles, alpha of every frame]
//   [workspace form only: per utterance 2 * S doubles]
struct FbPlan {
  int threads;  // as the alignment: 64 up to 64 states, 256 up to 1024, 1024 above
  bool lds, alpha_in_lds, row_in_lds;
  size_t lds_bytes;
  int max_states;
  size_t desc_bytes, alpha_doubles, vec_doubles, bytes;
  std::vector<AlignFbUtt> utts;
};

int fb_plan(const tdnnf_align_graphs *g, int num_utts, const int *utt_graph, const int *utt_frames, const int *utt_row_begin, bool post, FbPlan *p) {
  TDNNF_REQUIRE(g && num_utts > 0 && utt_frames, "align_posteriors: null graphs, no utterances or null utt_frames");
  TDNNF_REQUIRE(utt_graph || g->G == 1 || g->G == num_utts, "align_posteriors: utt_graph may be null only for one graph or one graph per utterance");
  p->utts.resize(num_utts);
  p->max_states = 0;
  size_t alpha = 0, vec = 0;
  long long rows = 0;
  for (int u = 0; u < num_utts; u++) {
    const int gi = utt_graph ? utt_graph[u] : g->G == 1 ? 0 : u;
    TDNNF_REQUIRE(gi >= 0 && gi < g->G, "align_posteriors: utterance %d names graph %d of %d", u, gi, g->G);
    TDNNF_REQUIRE(utt_frames[u] >= 0, "align_posteriors: utterance %d has %d frames", u, utt_frames[u]);
    const int S = g->state_begin[gi + 1] - g->state_begin[gi];
    p->max_states = std::max(p->max_states, S);
    AlignFbUtt &d = p->utts[u];
    d.graph = gi;
    d.frames = utt_frames[u];
    d.row_begin = utt_row_begin ? utt_row_begin[u] : 0;
    d.pad = 0;
    d.alpha_begin = (long long)alpha;
    d.vec_begin = (long long)vec;
    rows += utt_frames[u];
    TDNNF_REQUIRE(rows + num_utts < (1ll << 31), "align_posteriors: more than 2^31 frames in one call");
    alpha += ((size_t)utt_frames[u] + 1) * (size_t)S;
    vec += 2 * (size_t)S;
  }
  const size_t S8 = sizeof(double) * (size_t)p->max_states, rows_bytes = 2 * sizeof(float) * (size_t)g->P;
  const bool fits = 2 * S8 <= kLdsBudget;
  const int form = options().align_form;
  TDNNF_REQUIRE(form >= 0 && form <= 2, "align_posteriors: option align_form must be 0, 1 or 2");
  TDNNF_REQUIRE(form != 1 || fits, "align_posteriors: option align_form = 1, but two vectors of %d doubles do not fit the LDS", p->max_states);
  p->lds = form == 1 || (form == 0 && fits);
  p->threads = p->max_states <= 64 ? 64 : p->max_states <= 1024 ? 256 : 1024;
  p->alpha_in_lds = post && p->lds && 3 * S8 <= kLdsBudget && p->max_states <= kAlignFbAlphaRegs * p->threads;
  const size_t vec_bytes = (p->alpha_in_lds ? 3 : 2) * S8;
  // (with posteriors the rows are staged only behind a staged alpha_t: one launch form fewer, and a graph whose third vector does not fit has
  // little room left for rows)
  p->row_in_lds = p->lds && (!post || p->alpha_in_lds) && g->P <= kAlignRowRegs * p->threads && vec_bytes + rows_bytes <= kLdsBudget;
  p->lds_bytes = p->lds ? vec_bytes + (p->row_in_lds ? rows_bytes : 0) : 0;
  p->desc_bytes = round_up(sizeof(AlignFbUtt) * (size_t)num_utts, 256);
  p->alpha_doubles = post ? alpha : 0;
  p->vec_doubles = p->lds ? 0 : vec;
  p->bytes = 16 + p->desc_bytes + sizeof(double) * (p->alpha_doubles + p->vec_doubles);
  return TDNNF_OK;
}

struct FbArgs {
  AlignDev dev;
  AlignFbDev fb;
  const AlignFbUtt *utts;
  MatView y, post;
  int row_stride;
  float acoustic_scale, weight;
  double *alpha, *vecs, *results;
  int P;
};

template <int NT, bool LDS, bool YLDS, bool ALDS, bool POST>
int fb_launch_form(const FbPlan &p, const FbArgs &a, hipStream_t s) {
  if (LDS)
    TDNNF_HIP(hipFuncSetAttribute((const void *)align_fb_kernel<NT, LDS, YLDS, ALDS, POST>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes));
  hipLaunchKernelGGL((align_fb_kernel<NT, LDS, YLDS, ALDS, POST>), dim3((int)p.utts.size()), dim3(NT), p.lds_bytes, s, a.dev, a.fb, a.utts, a.y, a.row_stride,
                     a.acoustic_scale, a.weight, a.post, a.alpha, a.vecs, a.results, p.max_states, a.P);
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

template <int NT>
int fb_launch(const FbPlan &p, bool post, const FbArgs &a, hipStream_t s) {
  if (post) {
    if (p.row_in_lds) return fb_launch_form<NT, true, true, true, true>(p, a, s);
    if (p.alpha_in_lds) return fb_launch_form<NT, true, false, true, true>(p, a, s);
    if (p.lds) return fb_launch_form<NT, true, false, false, true>(p, a, s);
    return fb_launch_form<NT, false, false, false, true>(p, a, s);
  }
  if (p.row_in_lds) return fb_launch_form<NT, true, true, false, false>(p, a, s);
  if (p.lds) return fb_launch_form<NT, true, false, false, false>(p, a, s);
  return fb_launch_form<NT, false, false, false, false>(p, a, s);
}

}  // namespace

int align_fb_tables_create(tdnnf_align_graphs *g, const int *graph_state_begin, const int *graph_arc_begin, const int *arc_src, const int *arc_dst,
                           const int *arc_pdf, const float *arc_logprob) {
  FbHostTable by_src, by_pdf;
  std::vector<AlignFbGraphDev> gd(g->G);
  for (int k = 0; k < g->G; k++) {
    const int s0 = graph_state_begin[k], S = graph_state_begin[k + 1] - s0;
    std::vector<std::vector<int>> out(S), of_pdf(g->P);
    for (int a = graph_arc_begin[k]; a < graph_arc_begin[k + 1]; a++) {
      out[arc_src[a] - s0].push_back(a);
      of_pdf[arc_pdf[a]].push_back(a);
    }
    auto bits = [&](int a) {
      int b;
      memcpy(&b, &arc_logprob[a], 4);
      return b;
    };
    fb_add_graph(by_src, out, false, [&](int a) { return make_int4(arc_dst[a] - s0, arc_pdf[a], bits(a), a); }, &gd[k].src_slot0, &gd[k].src_num_slots,
                 &gd[k].src_heavy0, &gd[k].src_num_heavy);
    fb_add_graph(by_pdf, of_pdf, true, [&](int a) { return make_int4(arc_src[a] - s0, arc_dst[a] - s0, bits(a), a); }, &gd[k].pdf_slot0,
                 &gd[k].pdf_num_slots, &gd[k].pdf_heavy0, &gd[k].pdf_num_heavy);
  }
  TDNNF_REQUIRE(by_src.arcs.size() < (size_t)1 << 31 && by_pdf.arcs.size() < (size_t)1 << 31,
                "align_graphs_create: a sliced arc table (by source, by pdf) has more than 2^31 entries");
  int rc;
  if ((rc = fb_to_device(gd, &g->fb_graphs)) || (rc = fb_to_device(by_src.slots, &g->src_slots)) || (rc = fb_to_device(by_src.heavy, &g->src_heavy)) ||
      (rc = fb_to_device(by_src.arcs, &g->src_arcs)) || (rc = fb_to_device(by_pdf.slots, &g->pdf_slots)) ||
      (rc = fb_to_device(by_pdf.heavy, &g->pdf_heavy)) || (rc = fb_to_device(by_pdf.arcs, &g->pdf_arcs)))
    return rc;
  return TDNNF_OK;
}

void align_fb_tables_free(tdnnf_align_graphs *g) {
  void *ptrs[] = {g->fb_graphs, g->src_slots, g->src_heavy, g->src_arcs, g->pdf_slots, g->pdf_heavy, g->pdf_arcs};
  for (void *p : ptrs) (void)hipFree(p);
}

}  // namespace tdnnf

using namespace tdnnf;

extern "C" {

size_t tdnnf_align_posteriors_workspace_bytes(const tdnnf_align_graphs *g, int num_utts, const int *utt_graph, const int *utt_frames,
                                              int want_posteriors) {
  FbPlan p;
  if (fb_plan(g, num_utts, utt_graph, utt_frames, nullptr, want_posteriors != 0, &p) != TDNNF_OK) return 0;
  return p.bytes;
}

int tdnnf_align_posteriors(const tdnnf_align_graphs *g, int num_utts, const int *utt_graph, const int *utt_frames, const int *utt_row_begin,
                           int row_stride, const tdnnf_mat *nnet_output, float acoustic_scale, float weight, tdnnf_mat *post_out, double *results_dev,
                           void *workspace_dev, size_t workspace_bytes, tdnnf_stream stream) {
  TDNNF_REQUIRE(g && utt_row_begin && mat_ok(nnet_output) && results_dev && workspace_dev && (!post_out || mat_ok(post_out)),
                "align_posteriors: bad arguments");
  TDNNF_REQUIRE(row_stride >= 1, "align_posteriors: row_stride %d", row_stride);
  TDNNF_REQUIRE(nnet_output->cols >= g->P, "align_posteriors: nnet_output has %d columns, the graphs %d pdfs", nnet_output->cols, g->P);
  TDNNF_REQUIRE(!post_out || post_out->cols >= g->P, "align_posteriors: post_out has %d columns, the graphs %d pdfs", post_out ? post_out->cols : 0, g->P);
  const bool post = post_out != nullptr;
  FbPlan p;
  int rc = fb_plan(g, num_utts, utt_graph, utt_frames, utt_row_begin, post, &p);
  if (rc) return rc;
  for (int u = 0; u < num_utts; u++) {
    const long long last = (long long)utt_row_begin[u] + (long long)(utt_frames[u] - 1) * row_stride;
    TDNNF_REQUIRE(utt_row_begin[u] >= 0 && (utt_frames[u] == 0 || last < nnet_output->rows),
                  "align_posteriors: utterance %d reads rows %d .. %lld of a matrix of %d rows", u, utt_row_begin[u], last, nnet_output->rows);
    TDNNF_REQUIRE(!post || utt_frames[u] == 0 || last < post_out->rows,
                  "align_posteriors: utterance %d writes rows %d .. %lld of a post_out of %d rows", u, utt_row_begin[u], last, post ? post_out->rows : 0);
  }
  TDNNF_REQUIRE(workspace_bytes >= p.bytes, "align_posteriors: workspace of %zu bytes, %zu needed (tdnnf_align_posteriors_workspace_bytes)",
                workspace_bytes, p.bytes);
  hipStream_t s = (hipStream_t)stream;
  char *base = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(workspace_dev) + 15) & ~(uintptr_t)15);
  FbArgs a;
  AlignFbUtt *utts = reinterpret_cast<AlignFbUtt *>(base);
  a.utts = utts;
  a.alpha = reinterpret_cast<double *>(base + p.desc_bytes);
  a.vecs = a.alpha + p.alpha_doubles;
  // (pageable source: the runtime has taken the table by the time the call returns)
  TDNNF_HIP(hipMemcpyAsync(utts, p.utts.data(), sizeof(AlignFbUtt) * (size_t)num_utts, hipMemcpyHostToDevice, s));
  a.dev = AlignDev{g->graphs, g->slots, g->heavy, g->arcs, g->init, g->final};
  a.fb = AlignFbDev{g->fb_graphs, AlignFbTable{g->src_slots, g->src_heavy, g->src_arcs}, AlignFbTable{g->pdf_slots, g->pdf_heavy, g->pdf_arcs}};
  a.y = view(nnet_output);
  a.post = post ? view(post_out) : MatView{nullptr, 0, 0, 0};
  a.row_stride = row_stride;
  a.acoustic_scale = acoustic_scale;
  a.weight = weight;
  a.results = results_dev;
  a.P = g->P;
  switch (p.threads) {
    case 64:
      return fb_launch<64>(p, post, a, s);
    case 256:
      return fb_launch<256>(p, post, a, s);
    default:
      return fb_launch<1024>(p, post, a, s);
  }
}

}  // extern "C"
