// align_fb.hip -- forward-backward over pdf-labelled graphs (include/tdnnf_hip.h, "forward-backward") through a tdnnf_align_graphs
// (align_graphs.hip): sizes and lays out the workspace, launches align_fb_kernel (align_fb_kernels.h).
#include "align_fb_kernels.h"
#include "chain_plan.h"

namespace tdnnf {
namespace {

// What a call runs as and where its arrays lie behind the (16-byte aligned) start of the workspace:
//   [AlignUtt x num_utts, padded to 256 bytes] [posteriors: per utterance (frames + 1) * S doubles, alpha of every frame]
//   [workspace form only: per utterance 2 * S doubles]
struct FbPlan : AlignCall, AlignFormPlan {
  size_t alpha_doubles, bytes;
};

int fb_plan(const tdnnf_align_graphs *g, int num_utts, const int *utt_graph, const int *utt_frames, const int *utt_row_begin, int row_stride,
            const tdnnf_mat *nnet_output, const tdnnf_mat *post_out, bool post, FbPlan *p) {
  int rc = align_call(g, false, "align_posteriors: ", "align_posteriors: ", num_utts, utt_graph, utt_frames, utt_row_begin, row_stride, nnet_output,
                      post_out, p);
  if (rc) return rc;
  std::string err;
  TDNNF_REQUIRE(align_form_plan(p->max_states, g->P, options().align_form, post, kLdsBudget, "align_posteriors: ", p, &err), "%s", err.c_str());
  p->alpha_doubles = post ? p->frame_elems : 0;
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
};

template <int NT, bool LDS, bool YLDS, bool ALDS, bool POST>
int fb_launch_form(const FbPlan &p, const FbArgs &a, hipStream_t s) {
  if (LDS)
    TDNNF_HIP(hipFuncSetAttribute((const void *)align_fb_kernel<NT, LDS, YLDS, ALDS, POST>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes));
  hipLaunchKernelGGL((align_fb_kernel<NT, LDS, YLDS, ALDS, POST>), dim3((int)p.utts.size()), dim3(NT), p.lds_bytes, s, a.dev, a.utts, a.y, a.row_stride,
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
}  // namespace tdnnf

using namespace tdnnf;

extern "C" {

size_t tdnnf_align_posteriors_workspace_bytes(const tdnnf_align_graphs *g, int num_utts, const int *utt_graph, const int *utt_frames,
                                              int want_posteriors) {
  FbPlan p;
  if (fb_plan(g, num_utts, utt_graph, utt_frames, nullptr, 1, nullptr, nullptr, want_posteriors != 0, &p) != TDNNF_OK) return 0;
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
  int rc = fb_plan(g, num_utts, utt_graph, utt_frames, utt_row_begin, row_stride, nnet_output, post_out, post, &p);
  if (rc) return rc;
  TDNNF_REQUIRE(workspace_bytes >= p.bytes, "align_posteriors: workspace of %zu bytes, %zu needed (tdnnf_align_posteriors_workspace_bytes)",
                workspace_bytes, p.bytes);
  hipStream_t s = (hipStream_t)stream;
  char *base = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(workspace_dev) + 15) & ~(uintptr_t)15);
  FbArgs a;
  AlignUtt *utts = reinterpret_cast<AlignUtt *>(base);
  a.utts = utts;
  a.alpha = reinterpret_cast<double *>(base + p.desc_bytes);
  a.vecs = a.alpha + p.alpha_doubles;
  // (pageable source: the runtime has taken the table by the time the call returns)
  TDNNF_HIP(hipMemcpyAsync(utts, p.utts.data(), sizeof(AlignUtt) * (size_t)num_utts, hipMemcpyHostToDevice, s));
  a.dev = g->dev;
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
