// align.hip -- best-path alignment (include/tdnnf_hip.h, "best-path alignment") through a tdnnf_align_graphs (align_graphs.hip): sizes and lays
// out the workspace, launches align_best_path_kernel and, for the labelled call, align_path_labels_kernel behind it (align_kernels.h) -- under
// option align_path_checkpoint their *_ckpt_kernel twins, which keep the back-pointers of one segment of frames at a time.
#include "align_kernels.h"
#include "chain_plan.h"

namespace tdnnf {
namespace {

// What a call runs as and where its arrays lie behind the (16-byte aligned) start of the workspace:
//   [AlignUtt x num_utts, padded to 256 bytes] [back-pointers: per utterance frames * S ints, padded to an even count]
//   [global form only: per utterance 2 * S doubles]
// Under option align_path_checkpoint the second region holds per utterance the checkpoints, the segment buffer and the path of
// AlignPathCheckpointPlan (align_tables.h) instead, counted in ints as the back-pointers are.
struct AlignPlan : AlignCall, AlignFormPlan {
  AlignPathCheckpointPlan ckpt;
  size_t bytes;
};

// call: the prefix of the messages about the call's rows, the call's name
int align_plan(const tdnnf_align_graphs *g, const char *call, int num_utts, const int *utt_graph, const int *utt_frames, const int *utt_row_begin,
               int row_stride, const tdnnf_mat *nnet_output, AlignPlan *p) {
  int rc = align_call(g, true, "align: ", call, num_utts, utt_graph, utt_frames, utt_row_begin, row_stride, nnet_output, nullptr, p);
  if (rc) return rc;
  std::string err;
  TDNNF_REQUIRE(align_form_plan(p->max_states, g->P, options().align_form, false, kLdsBudget, "align: ", p, &err), "%s", err.c_str());
  int longest = 0;
  for (const AlignUtt &u : p->utts) longest = std::max(longest, u.frames);
  TDNNF_REQUIRE(align_path_checkpoint_plan(options().align_path_checkpoint, longest, call, &p->ckpt, &err), "%s", err.c_str());
  if (p->ckpt.C > 0) {
    p->frame_elems = 0;
    for (AlignUtt &u : p->utts) {
      u.frame_begin = (long long)p->frame_elems;
      p->frame_elems += p->ckpt.ints(u.frames, g->state_begin[u.graph + 1] - g->state_begin[u.graph]);
    }
  }
  if (p->lds) p->vec_doubles = 0;
  p->bytes = 16 + p->desc_bytes + sizeof(int) * p->frame_elems + sizeof(double) * p->vec_doubles;
  return TDNNF_OK;
}

template <int NT, bool LDS, bool YLDS>
int align_launch_form(const AlignPlan &p, int P, const AlignDev &dev, const AlignUtt *utts, const MatView &y, int row_stride, float acoustic_scale, int *bp,
                      double *vecs, int *pdf_out, int *state_out, double *results, hipStream_t s) {
  if (p.ckpt.C > 0) {  // (the same launch; the interval behind the other arguments)
    if (LDS)
      TDNNF_HIP(hipFuncSetAttribute((const void *)align_best_path_ckpt_kernel<NT, LDS, YLDS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes));
    hipLaunchKernelGGL((align_best_path_ckpt_kernel<NT, LDS, YLDS>), dim3((int)p.utts.size()), dim3(NT), p.lds_bytes, s, dev, utts, y, row_stride,
                       acoustic_scale, bp, vecs, pdf_out, state_out, results, p.max_states, P, p.ckpt.C);
    TDNNF_LAUNCH_CHECK();
    return TDNNF_OK;
  }
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

constexpr int kAlignLabelThreads = 256;

// tdnnf_align_best_path (label_out_dev null) and tdnnf_align_best_path_labels.  who: the prefix of the messages, the call's name.
int align_best_path(const tdnnf_align_graphs *g, const char *who, int num_utts, const int *utt_graph, const int *utt_frames, const int *utt_row_begin,
                    int row_stride, const tdnnf_mat *nnet_output, float acoustic_scale, int *pdf_out_dev, int *state_out_dev, int *label_out_dev,
                    int *arc_out_dev, double *results_dev, void *workspace_dev, size_t workspace_bytes, hipStream_t s) {
  TDNNF_REQUIRE(g && utt_row_begin && mat_ok(nnet_output) && pdf_out_dev && results_dev && workspace_dev, "%sbad arguments", who);
  TDNNF_REQUIRE(row_stride >= 1, "%srow_stride %d", who, row_stride);
  TDNNF_REQUIRE(nnet_output->cols >= g->P, "%snnet_output has %d columns, the graphs %d pdfs", who, nnet_output->cols, g->P);
  AlignPlan p;
  int rc = align_plan(g, who, num_utts, utt_graph, utt_frames, utt_row_begin, row_stride, nnet_output, &p);
  if (rc) return rc;
  TDNNF_REQUIRE(workspace_bytes >= p.bytes, "%sworkspace of %zu bytes, %zu needed (tdnnf_align_workspace_bytes)", who, workspace_bytes, p.bytes);
  char *base = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(workspace_dev) + 15) & ~(uintptr_t)15);
  AlignUtt *utts = reinterpret_cast<AlignUtt *>(base);
  int *bp = reinterpret_cast<int *>(base + p.desc_bytes);
  double *vecs = reinterpret_cast<double *>(base + p.desc_bytes + sizeof(int) * p.frame_elems);
  // (pageable source: the runtime has taken the table by the time the call returns)
  TDNNF_HIP(hipMemcpyAsync(utts, p.utts.data(), sizeof(AlignUtt) * (size_t)num_utts, hipMemcpyHostToDevice, s));
  const AlignDev &dev = g->dev;
  const MatView y = view(nnet_output);
  switch (p.threads) {
    case 64:
      rc = align_launch<64>(p, g->P, dev, utts, y, row_stride, acoustic_scale, bp, vecs, pdf_out_dev, state_out_dev, results_dev, s);
      break;
    case 256:
      rc = align_launch<256>(p, g->P, dev, utts, y, row_stride, acoustic_scale, bp, vecs, pdf_out_dev, state_out_dev, results_dev, s);
      break;
    default:
      rc = align_launch<1024>(p, g->P, dev, utts, y, row_stride, acoustic_scale, bp, vecs, pdf_out_dev, state_out_dev, results_dev, s);
  }
  if (rc || !label_out_dev) return rc;
  int max_frames = 0;
  for (int u = 0; u < num_utts; u++) max_frames = std::max(max_frames, utt_frames[u]);
  const int blocks = (max_frames + kAlignLabelThreads - 1) / kAlignLabelThreads;
  for (int u0 = 0; blocks > 0 && u0 < num_utts; u0 += 65535) {  // (a grid's second dimension ends at 65 535)
    if (p.ckpt.C > 0)
      hipLaunchKernelGGL(align_path_labels_ckpt_kernel<kAlignLabelThreads>, dim3(blocks, std::min(num_utts - u0, 65535)), dim3(kAlignLabelThreads), 0, s,
                         dev, utts + u0, bp, results_dev + 2 * (size_t)u0, g->arc_label_dev, label_out_dev, arc_out_dev, p.ckpt.C);
    else
      hipLaunchKernelGGL(align_path_labels_kernel<kAlignLabelThreads>, dim3(blocks, std::min(num_utts - u0, 65535)), dim3(kAlignLabelThreads), 0, s, dev,
                         utts + u0, bp, results_dev + 2 * (size_t)u0, g->arc_label_dev, label_out_dev, arc_out_dev);
    TDNNF_LAUNCH_CHECK();
  }
  return TDNNF_OK;
}

}  // namespace
}  // namespace tdnnf

using namespace tdnnf;

extern "C" {

size_t tdnnf_align_workspace_bytes(const tdnnf_align_graphs *g, int num_utts, const int *utt_graph, const int *utt_frames) {
  AlignPlan p;
  if (align_plan(g, "align_best_path: ", num_utts, utt_graph, utt_frames, nullptr, 1, nullptr, &p) != TDNNF_OK) return 0;
  return p.bytes;
}

int tdnnf_align_best_path(const tdnnf_align_graphs *g, int num_utts, const int *utt_graph, const int *utt_frames, const int *utt_row_begin,
                          int row_stride, const tdnnf_mat *nnet_output, float acoustic_scale, int *pdf_out_dev, int *state_out_dev,
                          double *results_dev, void *workspace_dev, size_t workspace_bytes, tdnnf_stream stream) {
  return align_best_path(g, "align_best_path: ", num_utts, utt_graph, utt_frames, utt_row_begin, row_stride, nnet_output, acoustic_scale, pdf_out_dev,
                         state_out_dev, nullptr, nullptr, results_dev, workspace_dev, workspace_bytes, (hipStream_t)stream);
}

int tdnnf_align_best_path_labels(const tdnnf_align_graphs *g, int num_utts, const int *utt_graph, const int *utt_frames, const int *utt_row_begin,
                                 int row_stride, const tdnnf_mat *nnet_output, float acoustic_scale, int *pdf_out_dev, int *state_out_dev,
                                 int *label_out_dev, int *arc_out_dev, double *results_dev, void *workspace_dev, size_t workspace_bytes,
                                 tdnnf_stream stream) {
  const char *who = "align_best_path_labels: ";
  int rc = align_need_labels(g, who);
  if (rc) return rc;
  TDNNF_REQUIRE(label_out_dev, "%snull label_out_dev", who);
  return align_best_path(g, who, num_utts, utt_graph, utt_frames, utt_row_begin, row_stride, nnet_output, acoustic_scale, pdf_out_dev, state_out_dev,
                         label_out_dev, arc_out_dev, results_dev, workspace_dev, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
