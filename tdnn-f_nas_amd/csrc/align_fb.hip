// align_fb.hip -- forward-backward over pdf-labelled graphs (include/tdnnf_hip.h, "forward-backward") through a tdnnf_align_graphs
// (align_graphs.hip): sizes and lays out the workspace, launches align_fb_kernel or, for the compact posteriors, align_fb_compact_kernel
// (per pdf) or align_fb_label_kernel (per label; align_fb_kernels.h) -- under option align_checkpoint their *_ckpt_kernel twins, which keep
// alpha of every C-th frame only.
#include <limits.h>

#include "align_fb_kernels.h"
#include "chain_plan.h"

namespace tdnnf {
namespace {

// What a call runs as and where its arrays lie behind the (16-byte aligned) start of the workspace:
//   [AlignUtt x num_utts, padded to 256 bytes] [posteriors: per utterance V * S doubles of alpha -- V = frames + 1, alpha of every frame,
//   or under option align_checkpoint the checkpoints and the segment buffer of AlignCheckpointPlan (align_tables.h)]
//   [workspace form only: per utterance 2 * S doubles]
struct FbPlan : AlignCall, AlignFormPlan {
  AlignCheckpointPlan ckpt;  // (C = 0 without posteriors: there is no alpha region to shorten)
  size_t alpha_doubles, bytes;
};

// who: the prefix of the messages, the call's name
int fb_plan(const tdnnf_align_graphs *g, const char *who, int num_utts, const int *utt_graph, const int *utt_frames, const int *utt_row_begin,
            int row_stride, const tdnnf_mat *nnet_output, const tdnnf_mat *post_out, bool post, FbPlan *p) {
  int rc = align_call(g, false, who, who, num_utts, utt_graph, utt_frames, utt_row_begin, row_stride, nnet_output, post_out, p);
  if (rc) return rc;
  std::string err;
  TDNNF_REQUIRE(align_form_plan(p->max_states, g->P, options().align_form, post, kLdsBudget, who, p, &err), "%s", err.c_str());
  int longest = 0;
  for (const AlignUtt &u : p->utts) longest = std::max(longest, u.frames);
  TDNNF_REQUIRE(align_checkpoint_plan(post ? options().align_checkpoint : 0, longest, who, &p->ckpt, &err), "%s", err.c_str());
  p->alpha_doubles = 0;
  if (post) {
    for (AlignUtt &u : p->utts) {
      u.frame_begin = (long long)p->alpha_doubles;
      p->alpha_doubles += p->ckpt.vectors(u.frames) * (size_t)(g->state_begin[u.graph + 1] - g->state_begin[u.graph]);
    }
  }
  if (p->lds) p->vec_doubles = 0;
  p->bytes = 16 + p->desc_bytes + sizeof(double) * (p->alpha_doubles + p->vec_doubles);
  return TDNNF_OK;
}

struct FbArgs {
  AlignDev dev;
  const AlignUtt *utts;
  MatView y, post;
  int row_stride;
  float acoustic_scale, weight;
  double *alpha, *vecs, *results;
  int P;
  float *compact;   // the compact form's output (post is unused then)
  const int *cols;  // its row width per graph
  AlignTable by_label;             // the label form: the fourth table
  const AlignRange *label_ranges;  // and the graphs' shares of it
};

// Sets up the workspace of a call whose plan is p -- the utterance table goes up on s -- and the arguments every form shares.
int fb_args(const tdnnf_align_graphs *g, const FbPlan &p, int row_stride, const tdnnf_mat *nnet_output, float acoustic_scale, float weight,
            double *results_dev, void *workspace_dev, hipStream_t s, FbArgs *a) {
  char *base = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(workspace_dev) + 15) & ~(uintptr_t)15);
  AlignUtt *utts = reinterpret_cast<AlignUtt *>(base);
  a->utts = utts;
  a->alpha = reinterpret_cast<double *>(base + p.desc_bytes);
  a->vecs = a->alpha + p.alpha_doubles;
  // (pageable source: the runtime has taken the table by the time the call returns)
  TDNNF_HIP(hipMemcpyAsync(utts, p.utts.data(), sizeof(AlignUtt) * p.utts.size(), hipMemcpyHostToDevice, s));
  a->dev = g->dev;
  a->y = view(nnet_output);
  a->post = MatView{nullptr, 0, 0, 0};
  a->row_stride = row_stride;
  a->acoustic_scale = acoustic_scale;
  a->weight = weight;
  a->results = results_dev;
  a->P = g->P;
  a->compact = nullptr;
  a->cols = g->num_cols_dev;
  a->by_label = AlignTable{};
  a->label_ranges = nullptr;
  return TDNNF_OK;
}

// One kernel of any form on the call's grid -- a workgroup of p.threads threads per utterance -- with the call's dynamic LDS.
template <class... P, class... A>
int fb_launch_kernel(void (*kernel)(P...), const FbPlan &p, hipStream_t s, A... args) {
  if (p.lds) TDNNF_HIP(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes));
  hipLaunchKernelGGL(kernel, dim3((int)p.utts.size()), dim3(p.threads), p.lds_bytes, s, args...);
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

// (under option align_checkpoint -- p.ckpt.C > 0 -- the *_ckpt_kernel of the same form, which takes the interval behind the other arguments)
template <int NT, bool LDS, bool YLDS, bool ALDS, bool POST>
int fb_launch_form(const FbPlan &p, const FbArgs &a, hipStream_t s) {
  if constexpr (POST) {  // (the forward-only forms keep no alpha and have no checkpointed twin)
    if (p.ckpt.C > 0)
      return fb_launch_kernel(align_fb_ckpt_kernel<NT, LDS, YLDS, ALDS>, p, s, a.dev, a.utts, a.y, a.row_stride, a.acoustic_scale, a.weight, a.post, a.alpha,
                              a.vecs, a.results, p.max_states, a.P, p.ckpt.C);
  }
  return fb_launch_kernel(align_fb_kernel<NT, LDS, YLDS, ALDS, POST>, p, s, a.dev, a.utts, a.y, a.row_stride, a.acoustic_scale, a.weight, a.post, a.alpha,
                          a.vecs, a.results, p.max_states, a.P);
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

template <int NT, bool LDS, bool YLDS, bool ALDS>
int fb_compact_launch_form(const FbPlan &p, const FbArgs &a, hipStream_t s) {
  if (p.ckpt.C > 0)
    return fb_launch_kernel(align_fb_compact_ckpt_kernel<NT, LDS, YLDS, ALDS>, p, s, a.dev, a.utts, a.y, a.row_stride, a.acoustic_scale, a.weight, a.compact,
                            a.cols, a.alpha, a.vecs, a.results, p.max_states, a.P, p.ckpt.C);
  return fb_launch_kernel(align_fb_compact_kernel<NT, LDS, YLDS, ALDS>, p, s, a.dev, a.utts, a.y, a.row_stride, a.acoustic_scale, a.weight, a.compact, a.cols,
                          a.alpha, a.vecs, a.results, p.max_states, a.P);
}

template <int NT>
int fb_compact_launch(const FbPlan &p, const FbArgs &a, hipStream_t s) {
  if (p.row_in_lds) return fb_compact_launch_form<NT, true, true, true>(p, a, s);
  if (p.alpha_in_lds) return fb_compact_launch_form<NT, true, false, true>(p, a, s);
  if (p.lds) return fb_compact_launch_form<NT, true, false, false>(p, a, s);
  return fb_compact_launch_form<NT, false, false, false>(p, a, s);
}

template <int NT, bool LDS, bool YLDS, bool ALDS>
int fb_label_launch_form(const FbPlan &p, const FbArgs &a, hipStream_t s) {
  if (p.ckpt.C > 0)
    return fb_launch_kernel(align_fb_label_ckpt_kernel<NT, LDS, YLDS, ALDS>, p, s, a.dev, a.by_label, a.label_ranges, a.utts, a.y, a.row_stride,
                            a.acoustic_scale, a.weight, a.compact, a.cols, a.alpha, a.vecs, a.results, p.max_states, a.P, p.ckpt.C);
  return fb_launch_kernel(align_fb_label_kernel<NT, LDS, YLDS, ALDS>, p, s, a.dev, a.by_label, a.label_ranges, a.utts, a.y, a.row_stride, a.acoustic_scale,
                          a.weight, a.compact, a.cols, a.alpha, a.vecs, a.results, p.max_states, a.P);
}

template <int NT>
int fb_label_launch(const FbPlan &p, const FbArgs &a, hipStream_t s) {
  if (p.row_in_lds) return fb_label_launch_form<NT, true, true, true>(p, a, s);
  if (p.alpha_in_lds) return fb_label_launch_form<NT, true, false, true>(p, a, s);
  if (p.lds) return fb_label_launch_form<NT, true, false, false>(p, a, s);
  return fb_label_launch_form<NT, false, false, false>(p, a, s);
}

// The compact layout of a call (include/tdnnf_hip.h): begin gets num_utts + 1 offsets in floats.  who: the prefix of the messages.
// labels: the rows are as wide as the graph's label column list, else as its pdf column list.
int fb_compact_layout(const tdnnf_align_graphs *g, bool labels, const char *who, int num_utts, const int *utt_graph, const int *utt_frames,
                      std::vector<long long> *begin) {
  int rc;
  if (labels && (rc = align_need_labels(g, who))) return rc;
  TDNNF_REQUIRE(g && num_utts > 0 && utt_frames, "%snull graphs, no utterances or null utt_frames", who);
  if ((rc = align_need_batch(g, who))) return rc;
  TDNNF_REQUIRE(utt_graph || g->G == 1 || g->G == num_utts, "%sutt_graph may be null only for one graph or one graph per utterance", who);
  begin->assign(1, 0);
  for (int u = 0; u < num_utts; u++) {
    const int gi = utt_graph ? utt_graph[u] : g->G == 1 ? 0 : u;
    TDNNF_REQUIRE(gi >= 0 && gi < g->G, "%sutterance %d names graph %d of %d", who, u, gi, g->G);
    TDNNF_REQUIRE(utt_frames[u] >= 0, "%sutterance %d has %d frames", who, u, utt_frames[u]);
    const std::vector<int> &cb = labels ? g->lcol_begin : g->col_begin;
    begin->push_back(begin->back() + (long long)utt_frames[u] * (cb[gi + 1] - cb[gi]));
  }
  return TDNNF_OK;
}

// tdnnf_align_posteriors_compact and tdnnf_align_label_posteriors_compact.  who: the prefix of the messages, the call's name.
int fb_compact(const tdnnf_align_graphs *g, bool labels, const char *who, int num_utts, const int *utt_graph, const int *utt_frames,
               const int *utt_row_begin, int row_stride, const tdnnf_mat *nnet_output, float acoustic_scale, float weight, float *post_compact_dev,
               size_t post_compact_elems, double *results_dev, void *workspace_dev, size_t workspace_bytes, tdnnf_stream stream) {
  int rc;
  if (labels && (rc = align_need_labels(g, who))) return rc;
  TDNNF_REQUIRE(g && utt_row_begin && mat_ok(nnet_output) && results_dev && workspace_dev, "%sbad arguments", who);
  TDNNF_REQUIRE(row_stride >= 1, "%srow_stride %d", who, row_stride);
  TDNNF_REQUIRE(nnet_output->cols >= g->P, "%snnet_output has %d columns, the graphs %d pdfs", who, nnet_output->cols, g->P);
  FbPlan p;
  if ((rc = fb_plan(g, who, num_utts, utt_graph, utt_frames, utt_row_begin, row_stride, nnet_output, nullptr, true, &p))) return rc;
  std::vector<long long> begin;
  if ((rc = fb_compact_layout(g, labels, who, num_utts, utt_graph, utt_frames, &begin))) return rc;
  const long long elems = begin.back();
  TDNNF_REQUIRE(post_compact_dev || elems == 0, "%snull post_compact_dev for an output of %lld floats", who, elems);
  TDNNF_REQUIRE(post_compact_elems >= (size_t)elems, "%spost_compact_elems %zu, the layout has %lld floats (tdnnf_align_%sposteriors_compact_layout)", who,
                post_compact_elems, elems, labels ? "label_" : "");
  for (int u = 0; u < num_utts; u++) {
    // (AlignUtt::out_begin is an int; an utterance that writes nothing needs no address)
    TDNNF_REQUIRE(begin[u + 1] == begin[u] || begin[u] <= INT_MAX,
                  "%sutterance %d's block starts at float %lld of the output, beyond the 2^31 - 1 a call can address: split the call", who, u, begin[u]);
    p.utts[u].out_begin = begin[u + 1] == begin[u] ? 0 : (int)begin[u];
  }
  TDNNF_REQUIRE(workspace_bytes >= p.bytes, "%sworkspace of %zu bytes, %zu needed (tdnnf_align_posteriors_workspace_bytes with want_posteriors)", who,
                workspace_bytes, p.bytes);
  hipStream_t s = (hipStream_t)stream;
  FbArgs a;
  if ((rc = fb_args(g, p, row_stride, nnet_output, acoustic_scale, weight, results_dev, workspace_dev, s, &a))) return rc;
  a.compact = post_compact_dev;
  if (labels) {
    a.cols = g->num_lcols_dev;
    a.by_label = g->by_label;
    a.label_ranges = g->label_range_dev;
    switch (p.threads) {
      case 64:
        return fb_label_launch<64>(p, a, s);
      case 256:
        return fb_label_launch<256>(p, a, s);
      default:
        return fb_label_launch<1024>(p, a, s);
    }
  }
  switch (p.threads) {
    case 64:
      return fb_compact_launch<64>(p, a, s);
    case 256:
      return fb_compact_launch<256>(p, a, s);
    default:
      return fb_compact_launch<1024>(p, a, s);
  }
}

// tdnnf_align_posteriors_compact_layout and tdnnf_align_label_posteriors_compact_layout: the layout into the caller's (optional) outputs
int fb_layout_out(const tdnnf_align_graphs *g, bool labels, const char *who, int num_utts, const int *utt_graph, const int *utt_frames,
                  long long *elems_out, long long *utt_begin_out) {
  std::vector<long long> begin;
  int rc = fb_compact_layout(g, labels, who, num_utts, utt_graph, utt_frames, &begin);
  if (rc) return rc;
  if (elems_out) *elems_out = begin.back();
  if (utt_begin_out) std::copy(begin.begin(), begin.end(), utt_begin_out);
  return TDNNF_OK;
}

}  // namespace
}  // namespace tdnnf

using namespace tdnnf;

extern "C" {

size_t tdnnf_align_posteriors_workspace_bytes(const tdnnf_align_graphs *g, int num_utts, const int *utt_graph, const int *utt_frames,
                                              int want_posteriors) {
  FbPlan p;
  if (fb_plan(g, "align_posteriors: ", num_utts, utt_graph, utt_frames, nullptr, 1, nullptr, nullptr, want_posteriors != 0, &p) != TDNNF_OK) return 0;
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
  int rc = fb_plan(g, "align_posteriors: ", num_utts, utt_graph, utt_frames, utt_row_begin, row_stride, nnet_output, post_out, post, &p);
  if (rc) return rc;
  TDNNF_REQUIRE(workspace_bytes >= p.bytes, "align_posteriors: workspace of %zu bytes, %zu needed (tdnnf_align_posteriors_workspace_bytes)",
                workspace_bytes, p.bytes);
  hipStream_t s = (hipStream_t)stream;
  FbArgs a;
  if ((rc = fb_args(g, p, row_stride, nnet_output, acoustic_scale, weight, results_dev, workspace_dev, s, &a))) return rc;
  if (post) a.post = view(post_out);
  switch (p.threads) {
    case 64:
      return fb_launch<64>(p, post, a, s);
    case 256:
      return fb_launch<256>(p, post, a, s);
    default:
      return fb_launch<1024>(p, post, a, s);
  }
}

int tdnnf_align_posteriors_compact_layout(const tdnnf_align_graphs *g, int num_utts, const int *utt_graph, const int *utt_frames, long long *elems_out,
                                          long long *utt_begin_out) {
  return fb_layout_out(g, false, "align_posteriors_compact_layout: ", num_utts, utt_graph, utt_frames, elems_out, utt_begin_out);
}

int tdnnf_align_posteriors_compact(const tdnnf_align_graphs *g, int num_utts, const int *utt_graph, const int *utt_frames, const int *utt_row_begin,
                                   int row_stride, const tdnnf_mat *nnet_output, float acoustic_scale, float weight, float *post_compact_dev,
                                   size_t post_compact_elems, double *results_dev, void *workspace_dev, size_t workspace_bytes, tdnnf_stream stream) {
  return fb_compact(g, false, "align_posteriors_compact: ", num_utts, utt_graph, utt_frames, utt_row_begin, row_stride, nnet_output, acoustic_scale, weight,
                    post_compact_dev, post_compact_elems, results_dev, workspace_dev, workspace_bytes, stream);
}

int tdnnf_align_label_posteriors_compact_layout(const tdnnf_align_graphs *g, int num_utts, const int *utt_graph, const int *utt_frames,
                                                long long *elems_out, long long *utt_begin_out) {
  return fb_layout_out(g, true, "align_label_posteriors_compact_layout: ", num_utts, utt_graph, utt_frames, elems_out, utt_begin_out);
}

int tdnnf_align_label_posteriors_compact(const tdnnf_align_graphs *g, int num_utts, const int *utt_graph, const int *utt_frames,
                                         const int *utt_row_begin, int row_stride, const tdnnf_mat *nnet_output, float acoustic_scale, float weight,
                                         float *post_compact_dev, size_t post_compact_elems, double *results_dev, void *workspace_dev,
                                         size_t workspace_bytes, tdnnf_stream stream) {
  return fb_compact(g, true, "align_label_posteriors_compact: ", num_utts, utt_graph, utt_frames, utt_row_begin, row_stride, nnet_output, acoustic_scale,
                    weight, post_compact_dev, post_compact_elems, results_dev, workspace_dev, workspace_bytes, stream);
}

}  // extern "C"
