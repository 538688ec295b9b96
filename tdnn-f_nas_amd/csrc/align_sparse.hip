// align_sparse.hip -- the sparse posteriors (include/tdnnf_hip.h, "sparse posteriors"): per frame the at most K (pdf, value) pairs above a
// floor -- or (label, value) pairs: the pdf and the label form share one plan and one body.  Runs the compact call (align_fb.hip) into a block of the workspace, then the selection pass over it (align_sparse_kernels.h) and
// the fold of its per-workgroup counts into the results.
#include <limits.h>
#include <math.h>

#include "align_sparse_kernels.h"

namespace tdnnf {
namespace {

// Where a call's arrays lie behind the (16-byte aligned) start of the workspace:
//   [the compact call's workspace, padded to 16 bytes] [its results: 2 doubles an utterance] [AlignSparseUtt x num_utts]
//   [one int2 per (utterance, group of kAlignSparseGroup frames)] [the compact block: elems floats]
struct SparsePlan {
  std::vector<AlignSparseUtt> utts;
  size_t fb_bytes;  // tdnnf_align_posteriors_workspace_bytes(..., 1)
  long long elems, frames, parts;
  int max_frames;
  size_t results_at, utts_at, parts_at, block_at, bytes;
};

// the refusal of a call made on this one's behalf, under this one's name
int sparse_refused(const char *who) {
  const std::string m = tdnnf_last_error();
  const size_t colon = m.find(": ");
  set_error("%s%s", who, colon == std::string::npos ? m.c_str() : m.c_str() + colon + 2);
  return TDNNF_EINVAL;
}

// labels: the block is the label compact call's and the columns are the graphs' label column lists
int sparse_plan(const tdnnf_align_graphs *g, bool labels, const char *who, int num_utts, const int *utt_graph, const int *utt_frames, int max_per_frame,
                SparsePlan *p) {
  int rc;
  if (labels && (rc = align_need_labels(g, who))) return rc;
  TDNNF_REQUIRE(max_per_frame >= 1 && max_per_frame <= kAlignSparseMaxK, "%smax_per_frame %d outside [1, %d]", who, max_per_frame, kAlignSparseMaxK);
  p->fb_bytes = tdnnf_align_posteriors_workspace_bytes(g, num_utts, utt_graph, utt_frames, 1);
  if (p->fb_bytes == 0) return sparse_refused(who);
  std::vector<long long> begin((size_t)num_utts + 1);
  const auto layout = labels ? tdnnf_align_label_posteriors_compact_layout : tdnnf_align_posteriors_compact_layout;
  if (layout(g, num_utts, utt_graph, utt_frames, &p->elems, begin.data()) != TDNNF_OK) return sparse_refused(who);
  const std::vector<int> &cb = labels ? g->lcol_begin : g->col_begin;
  p->utts.resize(num_utts);
  p->frames = p->parts = 0;
  p->max_frames = 0;
  for (int u = 0; u < num_utts; u++) {
    const int gi = utt_graph ? utt_graph[u] : g->G == 1 ? 0 : u;
    // (the compact call's limit, an int per block start, met here so that the workspace question answers it too)
    TDNNF_REQUIRE(begin[u + 1] == begin[u] || begin[u] <= INT_MAX,
                  "%sutterance %d's block starts at float %lld of the compact block, beyond the 2^31 - 1 a call can address: split the call", who, u, begin[u]);
    AlignSparseUtt &d = p->utts[u];
    d.block_begin = begin[u];
    d.frames = utt_frames[u];
    d.frame_begin = (int)p->frames;  // (below 2^31: the compact call's plan has checked the sum)
    d.D = cb[gi + 1] - cb[gi];
    d.col_begin = cb[gi];
    d.part_begin = (int)p->parts;
    d.pad = 0;
    p->frames += utt_frames[u];
    p->parts += (utt_frames[u] + kAlignSparseGroup - 1) / kAlignSparseGroup;
    p->max_frames = std::max(p->max_frames, utt_frames[u]);
  }
  p->results_at = align_round_up(p->fb_bytes, 16);
  p->utts_at = p->results_at + 2 * sizeof(double) * (size_t)num_utts;
  p->parts_at = p->utts_at + sizeof(AlignSparseUtt) * (size_t)num_utts;
  p->block_at = p->parts_at + sizeof(int2) * (size_t)p->parts;
  p->bytes = 16 + p->block_at + sizeof(float) * (size_t)p->elems;
  return TDNNF_OK;
}

// tdnnf_align_posteriors_sparse and tdnnf_align_label_posteriors_sparse.  who: the prefix of the messages, the call's name.  The selection
// kernels take a block, a column-list array and per-utterance (D, col_begin): they do not know which of the two they select from.
int sparse_call(const tdnnf_align_graphs *g, bool labels, const char *who, int num_utts, const int *utt_graph, const int *utt_frames,
                const int *utt_row_begin, int row_stride, const tdnnf_mat *nnet_output, float acoustic_scale, float weight, float min_post,
                int max_per_frame, int *pdf_out_dev, float *post_out_dev, int *count_out_dev, double *results_dev, void *workspace_dev,
                size_t workspace_bytes, tdnnf_stream stream) {
  TDNNF_REQUIRE(g && utt_row_begin && mat_ok(nnet_output) && results_dev && workspace_dev, "%sbad arguments", who);
  TDNNF_REQUIRE(isfinite(min_post) && min_post >= 0.f, "%smin_post %g must be finite and not negative", who, (double)min_post);
  SparsePlan p;
  int rc = sparse_plan(g, labels, who, num_utts, utt_graph, utt_frames, max_per_frame, &p);
  if (rc) return rc;
  TDNNF_REQUIRE(p.frames == 0 || (pdf_out_dev && post_out_dev && count_out_dev), "%snull pdf_out_dev, post_out_dev or count_out_dev for %lld frames", who,
                p.frames);
  TDNNF_REQUIRE(workspace_bytes >= p.bytes, "%sworkspace of %zu bytes, %zu needed (tdnnf_align_%sposteriors_sparse_workspace_bytes)", who, workspace_bytes,
                p.bytes, labels ? "label_" : "");
  char *base = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(workspace_dev) + 15) & ~(uintptr_t)15);
  double *fb_results = reinterpret_cast<double *>(base + p.results_at);
  AlignSparseUtt *utts = reinterpret_cast<AlignSparseUtt *>(base + p.utts_at);
  int2 *parts = reinterpret_cast<int2 *>(base + p.parts_at);
  float *block = reinterpret_cast<float *>(base + p.block_at);
  // the recursions: everything else the compact call refuses it refuses here, before anything is launched
  const auto compact = labels ? tdnnf_align_label_posteriors_compact : tdnnf_align_posteriors_compact;
  rc = compact(g, num_utts, utt_graph, utt_frames, utt_row_begin, row_stride, nnet_output, acoustic_scale, weight, block, (size_t)p.elems, fb_results, base,
               p.fb_bytes, stream);
  if (rc) return rc == TDNNF_EINVAL ? sparse_refused(who) : rc;
  hipStream_t s = (hipStream_t)stream;
  // (pageable source: the runtime has taken the table by the time the call returns)
  TDNNF_HIP(hipMemcpyAsync(utts, p.utts.data(), sizeof(AlignSparseUtt) * p.utts.size(), hipMemcpyHostToDevice, s));
  const int groups = (p.max_frames + kAlignSparseGroup - 1) / kAlignSparseGroup;
  for (int u0 = 0; groups > 0 && u0 < num_utts; u0 += 65535) {  // (a grid's second dimension ends at 65 535)
    hipLaunchKernelGGL(align_sparse_select_kernel, dim3(groups, std::min(num_utts - u0, 65535)), dim3(kAlignSparseWaves * 64), 0, s, utts + u0, block,
                       labels ? g->col_labels_dev : g->col_pdfs_dev, min_post, max_per_frame, pdf_out_dev, post_out_dev, count_out_dev, parts);
    TDNNF_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(align_sparse_results_kernel, dim3(num_utts), dim3(64), 0, s, utts, fb_results, parts, results_dev);
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

}  // namespace
}  // namespace tdnnf

using namespace tdnnf;

extern "C" {

size_t tdnnf_align_posteriors_sparse_workspace_bytes(const tdnnf_align_graphs *g, int num_utts, const int *utt_graph, const int *utt_frames,
                                                     int max_per_frame) {
  SparsePlan p;
  if (sparse_plan(g, false, "align_posteriors_sparse: ", num_utts, utt_graph, utt_frames, max_per_frame, &p) != TDNNF_OK) return 0;
  return p.bytes;
}

int tdnnf_align_posteriors_sparse(const tdnnf_align_graphs *g, int num_utts, const int *utt_graph, const int *utt_frames, const int *utt_row_begin,
                                  int row_stride, const tdnnf_mat *nnet_output, float acoustic_scale, float weight, float min_post, int max_per_frame,
                                  int *pdf_out_dev, float *post_out_dev, int *count_out_dev, double *results_dev, void *workspace_dev,
                                  size_t workspace_bytes, tdnnf_stream stream) {
  return sparse_call(g, false, "align_posteriors_sparse: ", num_utts, utt_graph, utt_frames, utt_row_begin, row_stride, nnet_output, acoustic_scale, weight,
                     min_post, max_per_frame, pdf_out_dev, post_out_dev, count_out_dev, results_dev, workspace_dev, workspace_bytes, stream);
}

size_t tdnnf_align_label_posteriors_sparse_workspace_bytes(const tdnnf_align_graphs *g, int num_utts, const int *utt_graph, const int *utt_frames,
                                                           int max_per_frame) {
  SparsePlan p;
  if (sparse_plan(g, true, "align_label_posteriors_sparse: ", num_utts, utt_graph, utt_frames, max_per_frame, &p) != TDNNF_OK) return 0;
  return p.bytes;
}

int tdnnf_align_label_posteriors_sparse(const tdnnf_align_graphs *g, int num_utts, const int *utt_graph, const int *utt_frames,
                                        const int *utt_row_begin, int row_stride, const tdnnf_mat *nnet_output, float acoustic_scale, float weight,
                                        float min_post, int max_per_frame, int *label_out_dev, float *post_out_dev, int *count_out_dev,
                                        double *results_dev, void *workspace_dev, size_t workspace_bytes, tdnnf_stream stream) {
  return sparse_call(g, true, "align_label_posteriors_sparse: ", num_utts, utt_graph, utt_frames, utt_row_begin, row_stride, nnet_output, acoustic_scale,
                     weight, min_post, max_per_frame, label_out_dev, post_out_dev, count_out_dev, results_dev, workspace_dev, workspace_bytes, stream);
}

}  // extern "C"
