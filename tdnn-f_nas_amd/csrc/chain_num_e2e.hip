// chain_num_e2e.hip -- the chain numerator on cyclic per-sequence graphs (flat-start / end-to-end LF-MMI): creates the second kind of
// tdnnf_supervision (its graphs are a tdnnf_align_graphs, its scratch its own) and launches num_e2e_kernels.h for the host functions of
// chain_num.hip, which dispatch on the supervision's kind.  tdnnf_supervision_reserve_e2e / _assign_e2e: the same kind allocated once for a
// capacity and given each minibatch in stream order, on a reserved graph set (align_graphs.hip).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <numeric>

#include "chain_plan.h"
#include "num_e2e_kernels.h"

namespace tdnnf {
namespace {

template <int NT, bool LDS, bool YLDS, bool FULL>
int e2e_launch_form(const tdnnf_supervision *sp, const MatView &y, double *num_lp, hipStream_t s) {
  if (LDS)
    TDNNF_HIP(hipFuncSetAttribute((const void *)num_e2e_recursion_kernel<NT, LDS, YLDS, FULL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sp->e2e_form.lds_bytes));
  hipLaunchKernelGGL((num_e2e_recursion_kernel<NT, LDS, YLDS, FULL>), dim3(sp->B), dim3(NT), sp->e2e_form.lds_bytes, s, sp->e2e_graphs->dev, y, sp->B, sp->T, sp->e2e_alpha,
                     sp->e2e_beta, sp->e2e_vecs, num_lp, sp->max_states_per_seq, sp->num_pdfs);
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

template <int NT, bool FULL>
int e2e_launch(const tdnnf_supervision *sp, const MatView &y, double *num_lp, hipStream_t s) {
  if (sp->e2e_form.row_in_lds) return e2e_launch_form<NT, true, true, FULL>(sp, y, num_lp, s);
  if (sp->e2e_form.lds) return e2e_launch_form<NT, true, false, FULL>(sp, y, num_lp, s);
  return e2e_launch_form<NT, false, false, FULL>(sp, y, num_lp, s);
}

template <bool FULL>
int e2e_recursion(const tdnnf_supervision *sp, const MatView &y, double *num_lp, hipStream_t s) {
  switch (sp->e2e_form.threads) {
    case 64:
      return e2e_launch<64, FULL>(sp, y, num_lp, s);
    case 256:
      return e2e_launch<256, FULL>(sp, y, num_lp, s);
    default:
      return e2e_launch<1024, FULL>(sp, y, num_lp, s);
  }
}

// the posterior pass: 256 threads, 1024 where the largest graph has more than 1024 states; alpha_t / beta_t+1 staged in LDS where the
// recursion's two vectors live there (the same 16 * Smax bytes)
template <int NT, bool LDS>
int e2e_posterior_form(const tdnnf_supervision *sp, int blocks, const MatView &y, const MatView &xent_out, const double *num_lp, const MatView &deriv,
                       const MatView &xent_deriv, float xent_scale, bool do_xent, hipStream_t s) {
  const size_t lds = LDS ? 2 * sizeof(double) * (size_t)sp->max_states_per_seq : 0;
  if (LDS) TDNNF_HIP(hipFuncSetAttribute((const void *)num_e2e_posterior_kernel<NT, LDS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((num_e2e_posterior_kernel<NT, LDS>), dim3(blocks, sp->B), dim3(NT), lds, s, sp->e2e_graphs->dev, y, xent_out, sp->B, sp->T, sp->weight, sp->e2e_alpha,
                     sp->e2e_beta, num_lp, deriv, xent_deriv, xent_scale, do_xent ? 1 : 0, sp->xent_part, sp->max_states_per_seq);
  return TDNNF_OK;
}

// What both assigns of a reserved end-to-end supervision check first, under the call's name `who`: the handle, the arguments (have_arrays:
// no array the call itself reads is null) and the two capacities beside the graph set's own.
int e2e_assign_check(const char *who, const tdnnf_supervision *sp, bool have_arrays, int B, int T) {
  TDNNF_REQUIRE(sp && sp->kind == 1 && sp->e2e_reserved, "%snot a supervision of tdnnf_supervision_reserve_e2e", who);
  TDNNF_REQUIRE(have_arrays && B > 0 && T > 0, "%sbad arguments", who);
  std::string err;
  TDNNF_REQUIRE(within_capacity(who, B, "sequences", sp->e2e_max_sequences, &err) && within_capacity(who, T, "frames", sp->e2e_max_frames, &err), "%s", err.c_str());
  return TDNNF_OK;
}

// The rest of both: the recursion's launch form from the minibatch's largest graph, then `assign`, the graph set's assign, and what follows
// from its return value.  A refusal left the graph set and so the supervision on the previous minibatch; an error of the runtime left the
// graph set with no batch (assign_stage.h), and the supervision then holds no minibatch either.  The totals are the graph set's.
template <class Assign>
int e2e_assign_finish(const char *who, tdnnf_supervision *sp, int B, int T, float weight, int max_states, Assign assign) {
  AlignFormPlan form;
  std::string err;
  TDNNF_REQUIRE(align_form_plan(max_states, sp->num_pdfs, options().align_form, false, kLdsBudget, who, &form, &err), "%s", err.c_str());
  const tdnnf_align_graphs *g = sp->e2e_graphs;
  if (int rc = assign()) {
    if (g->assigns == 0) sp->e2e_assigns = 0;
    return rc;
  }
  sp->B = B;
  sp->T = T;
  sp->weight = weight;
  sp->num_states = g->state_begin[B];
  sp->num_arcs = std::accumulate(g->num_arcs.begin(), g->num_arcs.end(), 0);
  sp->max_states_per_seq = sp->max_states_per_frame = max_states;
  sp->e2e_form = form;
  sp->e2e_assigns++;
  return TDNNF_OK;
}

}  // namespace

int num_e2e_recursion(const tdnnf_supervision *sp, const MatView &y, double *num_lp, bool forward_only, hipStream_t s) {
  TDNNF_REQUIRE(sp->num_pdfs <= y.cols, "chain numerator: the end-to-end supervision's num_pdfs %d exceeds nnet_output's %d columns", sp->num_pdfs, y.cols);
  return forward_only ? e2e_recursion<false>(sp, y, num_lp, s) : e2e_recursion<true>(sp, y, num_lp, s);
}

int num_e2e_posteriors(const tdnnf_supervision *sp, const MatView &y, const MatView &xent_out, const double *num_lp, double *xent_objf, const MatView &deriv,
                       const MatView &xent_deriv, float xent_scale, bool do_xent, hipStream_t s) {
  TDNNF_REQUIRE(sp->num_pdfs <= y.cols, "chain numerator: the end-to-end supervision's num_pdfs %d exceeds nnet_output's %d columns", sp->num_pdfs, y.cols);
  const int blocks = (sp->T + kNumE2eFrames - 1) / kNumE2eFrames;
  int rc;
  if (sp->max_states_per_seq > 1024)
    rc = sp->e2e_form.lds ? e2e_posterior_form<1024, true>(sp, blocks, y, xent_out, num_lp, deriv, xent_deriv, xent_scale, do_xent, s)
                     : e2e_posterior_form<1024, false>(sp, blocks, y, xent_out, num_lp, deriv, xent_deriv, xent_scale, do_xent, s);
  else
    rc = sp->e2e_form.lds ? e2e_posterior_form<256, true>(sp, blocks, y, xent_out, num_lp, deriv, xent_deriv, xent_scale, do_xent, s)
                     : e2e_posterior_form<256, false>(sp, blocks, y, xent_out, num_lp, deriv, xent_deriv, xent_scale, do_xent, s);
  if (rc) return rc;
  if (do_xent) hipLaunchKernelGGL(num_e2e_xent_sum_kernel, dim3((sp->B + 63) / 64), dim3(64), 0, s, sp->xent_part, sp->B, blocks, xent_objf);
  TDNNF_LAUNCH_CHECK();
  return TDNNF_OK;
}

}  // namespace tdnnf

using namespace tdnnf;

extern "C" {

int tdnnf_supervision_create_e2e(int B, int T, int num_pdfs, const int *seq_state_begin, const int *seq_arc_begin, const int *arc_src, const int *arc_dst,
                                 const int *arc_pdf, const float *arc_logprob, const float *initial_logprob, const float *final_logprob, float weight,
                                 tdnnf_supervision **out) {
  TDNNF_REQUIRE(out && B > 0 && T > 0 && num_pdfs > 0 && seq_state_begin && seq_arc_begin && arc_src && arc_dst && arc_pdf && arc_logprob && initial_logprob &&
                    final_logprob,
                "supervision_create_e2e: bad arguments");
  tdnnf_align_graphs *graphs = nullptr;
  // (validates what tdnnf_align_graphs_create validates: pdfs in [0, num_pdfs), states inside their sequence, an initial and a final state)
  int rc = tdnnf_align_graphs_create(B, num_pdfs, seq_state_begin, seq_arc_begin, arc_src, arc_dst, arc_pdf, arc_logprob, initial_logprob, final_logprob, &graphs);
  if (rc) return rc;
  tdnnf_supervision *sp = new tdnnf_supervision();
  memset(sp, 0, sizeof(*sp));
  sp->kind = 1;
  sp->B = B;
  sp->T = T;
  sp->weight = weight;
  sp->num_pdfs = num_pdfs;
  sp->e2e_graphs = graphs;
  sp->num_states = seq_state_begin[B];
  sp->num_arcs = seq_arc_begin[B];
  for (int s = 0; s < B; s++) sp->max_states_per_seq = std::max(sp->max_states_per_seq, seq_state_begin[s + 1] - seq_state_begin[s]);
  sp->max_states_per_frame = sp->max_states_per_seq;
  // the recursion's launch form, fixed here: the scratch depends on it
  std::string err;
  if (!align_form_plan(sp->max_states_per_seq, num_pdfs, options().align_form, false, kLdsBudget, "supervision_create_e2e: ", &sp->e2e_form, &err)) {
    tdnnf_supervision_destroy(sp);
    TDNNF_REQUIRE(false, "%s", err.c_str());
  }
  const size_t frames = sizeof(double) * ((size_t)T + 1) * (size_t)sp->num_states, parts = (size_t)B * ((T + kNumE2eFrames - 1) / kNumE2eFrames);
  hipError_t e = hipSuccess;
  if ((e = hipMalloc((void **)&sp->e2e_alpha, frames)) != hipSuccess || (e = hipMalloc((void **)&sp->e2e_beta, frames)) != hipSuccess ||
      (e = hipMalloc((void **)&sp->xent_part, sizeof(double) * parts)) != hipSuccess ||
      (e = hipMalloc((void **)&sp->l2_part, sizeof(double) * kFinishL2Parts)) != hipSuccess ||
      (!sp->e2e_form.lds && (e = hipMalloc((void **)&sp->e2e_vecs, 2 * sizeof(double) * (size_t)sp->num_states)) != hipSuccess)) {
    tdnnf_supervision_destroy(sp);
    return hip_status(e, "supervision_create_e2e: hipMalloc");
  }
  *out = sp;
  return TDNNF_OK;
}

int tdnnf_supervision_reserve_e2e(int max_sequences, int max_frames, int num_pdfs, int max_states, int max_arcs, tdnnf_supervision **out) {
  const char *who = "supervision_reserve_e2e: ";
  TDNNF_REQUIRE(out && max_sequences > 0 && max_frames > 0 && num_pdfs > 0 && max_states > 0 && max_arcs >= 0, "%sbad arguments", who);
  tdnnf_align_graphs *graphs = nullptr;
  int rc = tdnnf_align_graphs_reserve(max_sequences, num_pdfs, 0, max_states, max_arcs, &graphs);
  if (rc) return rc;
  tdnnf_supervision *sp = new tdnnf_supervision();
  memset(sp, 0, sizeof(*sp));
  sp->kind = 1;
  sp->num_pdfs = num_pdfs;
  sp->e2e_graphs = graphs;
  sp->e2e_reserved = true;
  sp->e2e_max_sequences = max_sequences;
  sp->e2e_max_frames = max_frames;
  // the scratch at the capacities; the two state vectors always, because the launch form follows the assigned minibatch
  const size_t frames = sizeof(double) * ((size_t)max_frames + 1) * (size_t)max_states;
  const size_t parts = (size_t)max_sequences * ((max_frames + kNumE2eFrames - 1) / kNumE2eFrames);
  hipError_t e = hipSuccess;
  if ((e = hipMalloc((void **)&sp->e2e_alpha, frames)) != hipSuccess || (e = hipMalloc((void **)&sp->e2e_beta, frames)) != hipSuccess ||
      (e = hipMalloc((void **)&sp->xent_part, sizeof(double) * parts)) != hipSuccess ||
      (e = hipMalloc((void **)&sp->l2_part, sizeof(double) * kFinishL2Parts)) != hipSuccess ||
      (e = hipMalloc((void **)&sp->e2e_vecs, 2 * sizeof(double) * (size_t)max_states)) != hipSuccess) {
    tdnnf_supervision_destroy(sp);
    return hip_status(e, "supervision_reserve_e2e: hipMalloc");
  }
  *out = sp;
  return TDNNF_OK;
}

int tdnnf_supervision_assign_e2e(tdnnf_supervision *sp, int B, int T, const int *seq_state_begin, const int *seq_arc_begin, const int *arc_src,
                                 const int *arc_dst, const int *arc_pdf, const float *arc_logprob, const float *initial_logprob, const float *final_logprob,
                                 float weight, tdnnf_stream stream) {
  const char *who = "supervision_assign_e2e: ";
  if (int rc = e2e_assign_check(who, sp, seq_state_begin && seq_arc_begin, B, T)) return rc;
  // this minibatch's largest graph (the graph set's assign refuses an array that is not what it seems)
  int max_states = 0;
  for (int s = 0; s < B; s++) max_states = std::max(max_states, seq_state_begin[s + 1] - seq_state_begin[s]);
  // (the assign validates what tdnnf_align_graphs_create validates and the capacities max_states and max_arcs; a refusal leaves everything as it was)
  return e2e_assign_finish(who, sp, B, T, weight, max_states, [&] {
    return tdnnf_align_graphs_assign(sp->e2e_graphs, B, seq_state_begin, seq_arc_begin, arc_src, arc_dst, arc_pdf, arc_logprob, initial_logprob, final_logprob, nullptr, stream);
  });
}

int tdnnf_supervision_assign_e2e_transcripts(tdnnf_supervision *sp, const tdnnf_unit_set *units, int B, int T, const int *slot_begin, const int *slot_unit,
                                             const int *slot_optional, float weight, tdnnf_stream stream) {
  const char *who = "supervision_assign_e2e_transcripts: ";
  if (int rc = e2e_assign_check(who, sp, units != nullptr, B, T)) return rc;
  // this minibatch's largest graph: the closed forms of align_transcripts.h, O(slots)
  std::string err;
  TDNNF_REQUIRE(transcripts_validate(who, units->host, B, slot_begin, slot_unit, slot_optional, &err), "%s", err.c_str());
  int max_states = 0;
  for (int s = 0, S, A; s < B; s++) {
    transcript_graph_size(units->host.context, slot_begin[s + 1] - slot_begin[s], slot_optional + slot_begin[s], &S, &A);
    max_states = std::max(max_states, S);
  }
  // (the assign checks the capacities max_states and max_arcs and the unit set's num_pdfs; a refusal leaves everything as it was)
  return e2e_assign_finish(who, sp, B, T, weight, max_states, [&] { return tdnnf_align_graphs_assign_transcripts(sp->e2e_graphs, units, B, slot_begin, slot_unit, slot_optional, stream); });
}

int tdnnf_supervision_assign_e2e_pronunciations(tdnnf_supervision *sp, const tdnnf_unit_set *units, int B, int T, const int *pos_begin, const int *pos_optional,
                                                const int *pos_alt_begin, const float *alt_logprob, const int *alt_unit_begin, const int *alt_units, float weight,
                                                tdnnf_stream stream) {
  const char *who = "supervision_assign_e2e_pronunciations: ";
  if (int rc = e2e_assign_check(who, sp, units != nullptr, B, T)) return rc;
  // this minibatch's largest graph: the closed forms of align_pronunciations.h
  const PronunciationBatch batch = {B, pos_begin, pos_optional, pos_alt_begin, alt_logprob, alt_unit_begin, alt_units};
  std::string err;
  TDNNF_REQUIRE(pronunciations_validate(who, units->host, batch, &err), "%s", err.c_str());
  long long max_states = 0;
  for (int s = 0; s < B; s++)
    max_states = std::max(max_states, pronunciation_graph_size(units->host.context, pos_begin[s + 1] - pos_begin[s], pos_optional + pos_begin[s],
                                                               pos_alt_begin + pos_begin[s], alt_unit_begin).states);
  TDNNF_REQUIRE(max_states < 1ll << 31, "%sa transcript has more than 2^31 states", who);
  // (the assign checks the capacities max_states and max_arcs and the unit set's num_pdfs; a refusal leaves everything as it was)
  return e2e_assign_finish(who, sp, B, T, weight, (int)max_states, [&] {
    return tdnnf_align_graphs_assign_pronunciations(sp->e2e_graphs, units, B, pos_begin, pos_optional, pos_alt_begin, alt_logprob, alt_unit_begin, alt_units, stream);
  });
}

int tdnnf_supervision_kind(const tdnnf_supervision *sp) {
  if (!sp) {
    set_error("supervision_kind: null supervision");
    return -1;
  }
  return sp->kind;
}

int tdnnf_supervision_e2e_form(const tdnnf_supervision *sp, int *threads, int *vectors_in_lds, int *rows_in_lds) {
  TDNNF_REQUIRE(sp && sp->kind == 1, "supervision_e2e_form: not an end-to-end supervision");
  if (threads) *threads = sp->e2e_form.threads;
  if (vectors_in_lds) *vectors_in_lds = sp->e2e_form.lds ? 1 : 0;
  if (rows_in_lds) *rows_in_lds = sp->e2e_form.row_in_lds ? 1 : 0;
  return TDNNF_OK;
}

}  // extern "C"
