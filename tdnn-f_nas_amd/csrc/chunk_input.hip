// chunk_input.hip -- the net's input for a minibatch of chunks, gathered on the device from whole utterances (tdnnf_chunk_input_*,
// include/tdnnf_hip.h "CHUNK INPUTS"): the t-major feature rows and the i-vector of every sequence, out of the stacked matrices
// tdnnf_infer_compute takes.  tdnnf_chunk_input_create makes every allocation once -- the device table and the two pinned staging buffers
// of assign_stage.h --, a gather validates on the host (chunk_input_plan.h), stages 16 bytes a sequence and enqueues one copy and one
// kernel (chunk_input_kernels.h) on the caller's stream: nothing allocated, nothing freed, no wait but the ring's for the copies of the
// turn before last.
#include <string>

#include "chunk_input_handle.h"
#include "chunk_input_kernels.h"

using namespace tdnnf;

extern "C" {

int tdnnf_chunk_input_create(int max_sequences, tdnnf_chunk_input **out) {
  const char *who = "chunk_input_create: ";
  TDNNF_REQUIRE(out && max_sequences >= 1 && max_sequences <= 1 << 24, "%sbad arguments (max_sequences %d)", who, max_sequences);
  tdnnf_chunk_input *h = new tdnnf_chunk_input();  // (zeroed)
  h->max_sequences = max_sequences;
  if (int rc = h->stage.create("chunk_input_create: allocation", sizeof(int) * kChunkTab * (size_t)max_sequences,
                               [h](Carve *c) { h->stage.dev = c->take<char>(h->stage.bytes); })) {
    tdnnf_chunk_input_destroy(h);
    return rc;
  }
  h->allocs_at_create = h->stage.device_allocs + h->stage.pinned_allocs;
  *out = h;
  return TDNNF_OK;
}

void tdnnf_chunk_input_destroy(tdnnf_chunk_input *h) {
  if (!h) return;
  h->stage.destroy();
  delete h;
}

int tdnnf_chunk_input_plan(int frame_subsampling, int frames_per_sequence, int num_sequences, const int *seq_utt_host, const int *chunk_begin_host,
                           int frame_shift, int num_utts, const int *frames_host, const int *ivector_rows_host, int ivector_period, int *table_out) {
  const char *who = "chunk_input_plan: ";
  TDNNF_REQUIRE(table_out, "%snull table_out", who);
  std::string err;
  // (i-vectors count unless the caller says there are none: a period > 0 without row counts)
  const bool use_iv = ivector_period <= 0 || ivector_rows_host;
  TDNNF_REQUIRE(chunk_input_plan(who, frame_subsampling, frames_per_sequence, num_sequences, seq_utt_host, chunk_begin_host, frame_shift, num_utts, frames_host,
                                 use_iv, ivector_rows_host, ivector_period, table_out, nullptr, &err),
                "%s", err.c_str());
  return TDNNF_OK;
}

int tdnnf_chunk_input_gather(tdnnf_chunk_input *h, int first_t, int num_t, int frame_subsampling, int frames_per_sequence, int num_sequences,
                             const int *seq_utt_host, const int *chunk_begin_host, int frame_shift, int num_utts, const int *frames_host,
                             const tdnnf_mat *feats, const int *ivector_rows_host, const tdnnf_mat *ivectors, int ivector_period, tdnnf_mat *feats_out,
                             tdnnf_mat *ivectors_out, tdnnf_stream stream) {
  const char *who = "chunk_input_gather: ";
  TDNNF_REQUIRE(h && mat_ok(feats) && mat_ok(feats_out), "%snull handle, or feats / feats_out missing or malformed", who);
  const int D = feats->cols;
  // ivector_dim 0 (no ivectors, or none of any width): no i-vector argument is read or written
  const bool use_iv = ivectors && ivectors->cols > 0;
  TDNNF_REQUIRE(!use_iv || (mat_ok(ivectors) && mat_ok(ivectors_out)), "%sivectors of %d columns need a well-formed ivectors_out", who, use_iv ? ivectors->cols : 0);
  TDNNF_REQUIRE(D >= 1 && num_t >= 1, "%sfeat_dim %d and num_t %d must be positive", who, D, num_t);
  std::string err;
  TDNNF_REQUIRE(within_capacity(who, num_sequences, "sequences", h->max_sequences, &err), "%s", err.c_str());
  ChunkInputRows rows;
  // the checks alone first: the staging buffer is taken only behind every refusal
  TDNNF_REQUIRE(chunk_input_plan(who, frame_subsampling, frames_per_sequence, num_sequences, seq_utt_host, chunk_begin_host, frame_shift, num_utts, frames_host,
                                 use_iv, ivector_rows_host, ivector_period, nullptr, &rows, &err),
                "%s", err.c_str());
  const int B = num_sequences;
  TDNNF_REQUIRE((long long)num_t * B < (1LL << 31), "%snum_t %d x %d sequences: too many rows", who, num_t, B);
  TDNNF_REQUIRE(feats->rows == rows.feat_rows, "%sfeats must be %lld x %d (the utterances stacked), not %d x %d", who, rows.feat_rows, D, feats->rows, feats->cols);
  TDNNF_REQUIRE(feats_out->rows == num_t * B && feats_out->cols == D, "%sfeats_out must be %d x %d (num_t x sequences rows), not %d x %d", who, num_t * B, D,
                feats_out->rows, feats_out->cols);
  if (use_iv) {
    TDNNF_REQUIRE(ivectors->rows == rows.ivector_rows, "%sivectors must be %lld x %d (the utterances' rows stacked), not %d x %d", who, rows.ivector_rows,
                  ivectors->cols, ivectors->rows, ivectors->cols);
    TDNNF_REQUIRE(ivectors_out->rows == B && ivectors_out->cols == ivectors->cols, "%sivectors_out must be %d x %d (a row a sequence), not %d x %d", who, B,
                  ivectors->cols, ivectors_out->rows, ivectors_out->cols);
  }

  StagePacker pk;
  if (int rc = h->stage.begin(&pk)) return rc;
  // the table straight into this turn's pinned buffer: 16 bytes a sequence
  int *table = reinterpret_cast<int *>(pk.host);
  chunk_input_plan(who, frame_subsampling, frames_per_sequence, B, seq_utt_host, chunk_begin_host, frame_shift, num_utts, frames_host, use_iv, ivector_rows_host,
                   ivector_period, table, nullptr, &err);
  pk.at = sizeof(int) * kChunkTab * (size_t)B;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = h->stage.submit(pk, pk.at, s)) return rc;
  const MatView none{nullptr, 0, 0, 0};
  const MatView fv = view(feats), ov = view(feats_out), ivv = use_iv ? view(ivectors) : none, iov = use_iv ? view(ivectors_out) : none;
  const bool v4 = vec4_ok(fv) && vec4_ok(ov) && (!use_iv || (vec4_ok(ivv) && vec4_ok(iov)));
  const int w = v4 ? 4 : 1;
  const long long work = (long long)ov.rows * (D / w) + (long long)B * (iov.cols / w);
  const int *tab = reinterpret_cast<const int *>(h->stage.dev);
  if (v4) hipLaunchKernelGGL(chunk_input_gather_kernel<4>, dim3(grid_for(work, 256)), dim3(256), 0, s, fv, ivv, tab, B, first_t, ov, iov);
  else hipLaunchKernelGGL(chunk_input_gather_kernel<1>, dim3(grid_for(work, 256)), dim3(256), 0, s, fv, ivv, tab, B, first_t, ov, iov);
  TDNNF_LAUNCH_CHECK();
  h->gathers++;
  h->last_form = w;
  return TDNNF_OK;
}

int tdnnf_chunk_input_info(const tdnnf_chunk_input *h, int *max_sequences, long long *allocations, long long *gathers, int *last_form) {
  TDNNF_REQUIRE(h, "chunk_input_info: null handle");
  if (max_sequences) *max_sequences = h->max_sequences;
  if (allocations) *allocations = h->stage.device_allocs + h->stage.pinned_allocs - h->allocs_at_create;
  if (gathers) *gathers = h->gathers;
  if (last_form) *last_form = h->last_form;
  return TDNNF_OK;
}

}  // extern "C"
