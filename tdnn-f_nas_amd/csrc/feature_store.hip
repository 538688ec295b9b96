// feature_store.hip -- utterances' features kept on the device as Kaldi's CompressedMatrix codes and decoded where they are read
// (tdnnf_feature_store_*, tdnnf_chunk_input_gather_stored; include/tdnnf_hip.h "FEATURE STORES").  tdnnf_feature_store_create makes every
// allocation once: one device arena -- the codes, the format-1 header floats, the table of utterances, the staging of an expand's list --
// and the two pinned buffers of assign_stage.h for that list.  An append validates and packs on the host (feature_store_plan.h) and copies
// behind the store's last byte, so nothing enqueued earlier reads what it writes; it waits for its copies.  An expand stages 8 bytes a list
// entry and enqueues one copy and one kernel a piece of kExpandPiece entries; the gather out of a store stages the minibatch's table
// through the chunk-input handle's ring and enqueues one copy and one kernel (feature_store_kernels.h).  Neither allocates or waits, but
// for the ring's copies of the turn before last.
#include <string>
#include <vector>

#include "chunk_input_handle.h"
#include "feature_store_kernels.h"

using namespace tdnnf;

struct tdnnf_feature_store {
  int format, feat_dim, max_utterances, max_frames;
  AssignStage stage;  // dev: the staged list of an expand, 2 ints an entry
  unsigned char *codes;
  float4 *headers;  // format 1 only
  StoreUtt *utts;
  std::vector<int> frames;  // of every utterance (reserved at create)
  long long total_frames, code_bytes;
  int allocs_at_create;
  long long gathers, expands;
  int last_form;  // of the last gather or expand: 4 the wide form, 1 a code at a time, 0 before the first
};

namespace {

// The entries of an expand's list staged a turn of the ring: the pinned buffers and the device staging take 8 bytes each, whatever the
// store's capacities.
constexpr int kExpandPiece = 1024;

StoreView view_of(const tdnnf_feature_store *h) { return StoreView{h->codes, h->headers, h->utts, h->feat_dim}; }

// One checked utterance of an append: its rows and global header.
struct Pending {
  int rows;
  float min_value, range;
};

// The capacity checks of an append of n utterances of `rows` frames in all (the words of within_capacity, for a 64-bit count).
bool append_fits(const char *who, const tdnnf_feature_store *h, int n, long long rows, std::string *err) {
  if (!within_capacity(who, (int)std::min<long long>((long long)h->frames.size() + n, 0x7fffffff), "utterances", h->max_utterances, err)) return false;
  const long long frames = h->total_frames + rows;
  if (frames <= h->max_frames) return true;
  char buf[256];
  snprintf(buf, sizeof(buf), "%s%lld frames exceed the capacity max_frames = %d by %lld", who, frames, h->max_frames, frames - h->max_frames);
  *err = buf;
  return false;
}

// Copies n checked utterances behind the store's last and commits them.  pack(i, header, codes): the header floats (format 1) and the
// row-major codes of utterance i into buffers of exactly their size.
template <class Pack>
int append_copy(tdnnf_feature_store *h, int n, const std::vector<Pending> &items, Pack pack) {
  const int D = h->feat_dim, U = (int)h->frames.size();
  std::vector<StoreUtt> table(n);
  std::vector<unsigned char> codes;
  std::vector<float> header(h->format == 1 ? 4 * (size_t)D : 0);
  long long at = h->code_bytes;
  for (int i = 0; i < n; i++) {
    table[i] = StoreUtt{at, items[i].rows, U + i, items[i].min_value, items[i].range, {0, 0}};
    codes.resize((size_t)items[i].rows * D * code_width(h->format));
    pack(i, header.data(), codes.data());
    TDNNF_HIP(hipMemcpy(h->codes + at, codes.data(), codes.size(), hipMemcpyHostToDevice));
    if (h->format == 1) TDNNF_HIP(hipMemcpy(h->headers + (size_t)(U + i) * D, header.data(), sizeof(float) * header.size(), hipMemcpyHostToDevice));
    at += utt_code_bytes(h->format, D, items[i].rows);
  }
  TDNNF_HIP(hipMemcpy(h->utts + U, table.data(), sizeof(StoreUtt) * (size_t)n, hipMemcpyHostToDevice));
  // committed only here: a failed copy leaves the store's utterances as they were, the bytes behind them unread
  for (int i = 0; i < n; i++) {
    h->frames.push_back(items[i].rows);
    h->total_frames += items[i].rows;
  }
  h->code_bytes = at;
  return TDNNF_OK;
}

FeaturePayload payload_of(const tdnnf_feature_payload &p) {
  return FeaturePayload{p.format, p.min_value, p.range, p.rows, p.cols, static_cast<const uint16_t *>(p.percentiles), p.codes};
}

template <template <int, int> class K, class... Args>
void launch_form(int format, bool v4, long long work, hipStream_t s, Args... args) {
  const dim3 grid(grid_for(work, 256)), block(256);
  if (format == 1) v4 ? K<1, 4>::launch(grid, block, s, args...) : K<1, 1>::launch(grid, block, s, args...);
  else if (format == 2) v4 ? K<2, 4>::launch(grid, block, s, args...) : K<2, 1>::launch(grid, block, s, args...);
  else v4 ? K<3, 4>::launch(grid, block, s, args...) : K<3, 1>::launch(grid, block, s, args...);
}
template <int FMT, int VEC>
struct Gather {
  static void launch(dim3 grid, dim3 block, hipStream_t s, StoreView st, MatView iv, const int *tab, int B, int first_t, MatView out, MatView iv_out) {
    hipLaunchKernelGGL((feature_store_gather_kernel<FMT, VEC>), grid, block, 0, s, st, iv, tab, B, first_t, out, iv_out);
  }
};
template <int FMT, int VEC>
struct Expand {
  static void launch(dim3 grid, dim3 block, hipStream_t s, StoreView st, const int *list, int n, MatView out) {
    hipLaunchKernelGGL((feature_store_expand_kernel<FMT, VEC>), grid, block, 0, s, st, list, n, out);
  }
};

}  // namespace

extern "C" {

int tdnnf_feature_store_create(int format, int feat_dim, int max_utterances, long long max_frames, tdnnf_feature_store **out) {
  const char *who = "feature_store_create: ";
  TDNNF_REQUIRE(out && store_format_ok(format), "%sformat %d: a store holds format 1 (CM), 2 (CM2) or 3 (CM3)", who, format);
  TDNNF_REQUIRE(feat_dim >= 1 && feat_dim <= 1 << 16 && max_utterances >= 1 && max_utterances <= 1 << 26 && max_frames >= 1 && max_frames < (1LL << 31),
                "%sbad arguments (feat_dim %d, max_utterances %d, max_frames %lld)", who, feat_dim, max_utterances, max_frames);
  tdnnf_feature_store *h = new tdnnf_feature_store();  // (zeroed)
  h->format = format;
  h->feat_dim = feat_dim;
  h->max_utterances = max_utterances;
  h->max_frames = (int)max_frames;
  h->frames.reserve(max_utterances);
  // the codes of max_frames frames, and at most 15 bytes of padding behind every utterance
  const size_t code_capacity = (size_t)max_frames * feat_dim * code_width(format) + 16 * (size_t)max_utterances;
  if (int rc = h->stage.create("feature_store_create: allocation", 2 * sizeof(int) * (size_t)kExpandPiece, [&](Carve *c) {
        h->codes = c->take<unsigned char>(code_capacity);
        h->headers = format == 1 ? c->take<float4>((size_t)max_utterances * feat_dim) : nullptr;
        h->utts = c->take<StoreUtt>(max_utterances);
        h->stage.dev = c->take<char>(h->stage.bytes);
      })) {
    tdnnf_feature_store_destroy(h);
    return rc;
  }
  h->allocs_at_create = h->stage.device_allocs + h->stage.pinned_allocs;
  *out = h;
  return TDNNF_OK;
}

void tdnnf_feature_store_destroy(tdnnf_feature_store *h) {
  if (!h) return;
  h->stage.destroy();
  delete h;
}

int tdnnf_feature_store_layout(int format, int feat_dim, int num_utts, const int *frames_host, long long *offsets_out, long long *device_bytes_out) {
  std::string err;
  TDNNF_REQUIRE(feature_store_layout("feature_store_layout: ", format, feat_dim, num_utts, frames_host, offsets_out, device_bytes_out, &err), "%s", err.c_str());
  return TDNNF_OK;
}

int tdnnf_feature_store_pack(int feat_dim, const tdnnf_feature_payload *item, float *header_out, void *codes_out) {
  const char *who = "feature_store_pack: ";
  TDNNF_REQUIRE(item && codes_out && (item->format != 1 || header_out), "%snull item, codes_out or (format 1) header_out", who);
  TDNNF_REQUIRE(store_format_ok(item->format), "%sformat %d: a payload is of format 1 (CM), 2 (CM2) or 3 (CM3)", who, item->format);
  const FeaturePayload p = payload_of(*item);
  std::string err;
  TDNNF_REQUIRE(feature_payload_check(who, 0, p.format, feat_dim, p, &err), "%s", err.c_str());
  feature_payload_pack(p, header_out, codes_out);
  return TDNNF_OK;
}

int tdnnf_feature_store_compress(int format, int rows, int cols, const float *matrix_host, float *min_out, float *range_out, void *codes_out) {
  const char *who = "feature_store_compress: ";
  TDNNF_REQUIRE(min_out && range_out && codes_out, "%snull min_out, range_out or codes_out", who);
  std::string err;
  float mn, range;
  TDNNF_REQUIRE(feature_compress_check(who, 0, format, rows, cols, matrix_host, &mn, &range, &err), "%s", err.c_str());
  feature_compress(format, rows, cols, matrix_host, mn, range, codes_out);
  *min_out = mn;
  *range_out = range;
  return TDNNF_OK;
}

int tdnnf_feature_store_append(tdnnf_feature_store *h, int num_items, const tdnnf_feature_payload *items) {
  const char *who = "feature_store_append: ";
  TDNNF_REQUIRE(h && items && num_items >= 1, "%snull handle or items, or no item (%d)", who, num_items);
  std::string err;
  std::vector<Pending> pending(num_items);
  long long rows = 0;
  for (int i = 0; i < num_items; i++) {
    TDNNF_REQUIRE(feature_payload_check(who, i, h->format, h->feat_dim, payload_of(items[i]), &err), "%s", err.c_str());
    pending[i] = Pending{items[i].rows, items[i].min_value, items[i].range};
    rows += items[i].rows;
  }
  TDNNF_REQUIRE(append_fits(who, h, num_items, rows, &err), "%s", err.c_str());
  return append_copy(h, num_items, pending, [&](int i, float *header, unsigned char *codes) { feature_payload_pack(payload_of(items[i]), header, codes); });
}

int tdnnf_feature_store_append_float(tdnnf_feature_store *h, int num_items, const int *rows_host, const float *matrices_host) {
  const char *who = "feature_store_append_float: ";
  TDNNF_REQUIRE(h && rows_host && num_items >= 1, "%snull handle or rows_host, or no item (%d)", who, num_items);
  std::string err;
  std::vector<Pending> pending(num_items);
  std::vector<const float *> first(num_items);
  long long rows = 0;
  for (int i = 0; i < num_items; i++) {
    first[i] = matrices_host ? matrices_host + (size_t)rows * h->feat_dim : nullptr;
    float mn = 0.f, range = 0.f;
    TDNNF_REQUIRE(feature_compress_check(who, i, h->format, rows_host[i], h->feat_dim, first[i], &mn, &range, &err), "%s", err.c_str());
    pending[i] = Pending{rows_host[i], mn, range};
    rows += rows_host[i];
  }
  TDNNF_REQUIRE(append_fits(who, h, num_items, rows, &err), "%s", err.c_str());
  return append_copy(h, num_items, pending, [&](int i, float *, unsigned char *codes) {
    feature_compress(h->format, pending[i].rows, h->feat_dim, first[i], pending[i].min_value, pending[i].range, codes);
  });
}

int tdnnf_feature_store_expand(tdnnf_feature_store *h, int num_utts, const int *utt_host, tdnnf_mat *out, tdnnf_stream stream) {
  const char *who = "feature_store_expand: ";
  TDNNF_REQUIRE(h && utt_host && num_utts >= 1 && mat_ok(out), "%snull handle or utt_host, no utterance (%d), or out missing or malformed", who, num_utts);
  const int U = (int)h->frames.size(), D = h->feat_dim;
  long long rows = 0;
  for (int i = 0; i < num_utts; i++) {
    TDNNF_REQUIRE(utt_host[i] >= 0 && utt_host[i] < U, "%sentry %d: utterance %d outside [0, %d)", who, i, utt_host[i], U);
    rows += h->frames[utt_host[i]];
  }
  TDNNF_REQUIRE(rows < (1LL << 31), "%s%lld rows: too many", who, rows);
  TDNNF_REQUIRE(out->rows == rows && out->cols == D, "%sout must be %lld x %d (the listed utterances stacked), not %d x %d", who, rows, D, out->rows, out->cols);
  const MatView ov = view(out);
  const bool v4 = vec4_ok(ov);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // a piece of at most kExpandPiece entries a turn of the ring: its list [utterance, first output row of the piece], one copy, one kernel
  for (int begin = 0, row0 = 0; begin < num_utts;) {
    const int n = std::min(num_utts - begin, kExpandPiece);
    StagePacker pk;
    if (int rc = h->stage.begin(&pk)) return rc;
    int *list = reinterpret_cast<int *>(pk.host), piece_rows = 0;
    for (int i = 0; i < n; i++) {
      list[2 * i] = utt_host[begin + i];
      list[2 * i + 1] = piece_rows;
      piece_rows += h->frames[utt_host[begin + i]];
    }
    pk.at = 2 * sizeof(int) * (size_t)n;
    if (int rc = h->stage.submit(pk, pk.at, s)) return rc;
    const MatView piece{ov.data + (size_t)row0 * ov.stride, piece_rows, D, ov.stride};
    launch_form<Expand>(h->format, v4, (long long)piece_rows * (D / (v4 ? 4 : 1)), s, view_of(h), reinterpret_cast<const int *>(h->stage.dev), n, piece);
    TDNNF_LAUNCH_CHECK();
    begin += n;
    row0 += piece_rows;
  }
  h->expands++;
  h->last_form = v4 ? 4 : 1;
  return TDNNF_OK;
}

int tdnnf_chunk_input_gather_stored(tdnnf_chunk_input *ci, int first_t, int num_t, int frame_subsampling, int frames_per_sequence, int num_sequences,
                                    const int *seq_utt_host, const int *chunk_begin_host, int frame_shift, tdnnf_feature_store *h,
                                    const int *ivector_rows_host, const tdnnf_mat *ivectors, int ivector_period, tdnnf_mat *feats_out, tdnnf_mat *ivectors_out,
                                    tdnnf_stream stream) {
  const char *who = "chunk_input_gather_stored: ";
  TDNNF_REQUIRE(ci && h && mat_ok(feats_out), "%snull handle or store, or feats_out missing or malformed", who);
  const int D = h->feat_dim, U = (int)h->frames.size();
  const bool use_iv = ivectors && ivectors->cols > 0;
  TDNNF_REQUIRE(!use_iv || (mat_ok(ivectors) && mat_ok(ivectors_out)), "%sivectors of %d columns need a well-formed ivectors_out", who, use_iv ? ivectors->cols : 0);
  TDNNF_REQUIRE(num_t >= 1, "%snum_t %d must be positive", who, num_t);
  TDNNF_REQUIRE(U >= 1, "%sthe store holds no utterance", who);
  std::string err;
  TDNNF_REQUIRE(within_capacity(who, num_sequences, "sequences", ci->max_sequences, &err), "%s", err.c_str());
  ChunkInputRows rows;
  // the checks of "CHUNK INPUTS" alone first, with the store's frames: the staging buffer is taken only behind every refusal
  TDNNF_REQUIRE(chunk_input_plan(who, frame_subsampling, frames_per_sequence, num_sequences, seq_utt_host, chunk_begin_host, frame_shift, U, h->frames.data(),
                                 use_iv, ivector_rows_host, ivector_period, nullptr, &rows, &err),
                "%s", err.c_str());
  const int B = num_sequences;
  TDNNF_REQUIRE((long long)num_t * B < (1LL << 31), "%snum_t %d x %d sequences: too many rows", who, num_t, B);
  TDNNF_REQUIRE(feats_out->rows == num_t * B && feats_out->cols == D, "%sfeats_out must be %d x %d (num_t x sequences rows), not %d x %d", who, num_t * B, D,
                feats_out->rows, feats_out->cols);
  if (use_iv) {
    TDNNF_REQUIRE(ivectors->rows == rows.ivector_rows, "%sivectors must be %lld x %d (the utterances' rows stacked), not %d x %d", who, rows.ivector_rows,
                  ivectors->cols, ivectors->rows, ivectors->cols);
    TDNNF_REQUIRE(ivectors_out->rows == B && ivectors_out->cols == ivectors->cols, "%sivectors_out must be %d x %d (a row a sequence), not %d x %d", who, B,
                  ivectors->cols, ivectors_out->rows, ivectors_out->cols);
  }

  StagePacker pk;
  if (int rc = ci->stage.begin(&pk)) return rc;
  // the table of the float gather, its first entry the utterance's index in the store instead of a stacked row
  int *table = reinterpret_cast<int *>(pk.host);
  chunk_input_plan(who, frame_subsampling, frames_per_sequence, B, seq_utt_host, chunk_begin_host, frame_shift, U, h->frames.data(), use_iv, ivector_rows_host,
                   ivector_period, table, nullptr, &err);
  for (int b = 0; b < B; b++) table[kChunkTab * b] = seq_utt_host[b];
  pk.at = sizeof(int) * kChunkTab * (size_t)B;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = ci->stage.submit(pk, pk.at, s)) return rc;
  const MatView none{nullptr, 0, 0, 0};
  const MatView ov = view(feats_out), ivv = use_iv ? view(ivectors) : none, iov = use_iv ? view(ivectors_out) : none;
  const bool v4 = vec4_ok(ov) && (!use_iv || (vec4_ok(ivv) && vec4_ok(iov)));
  const int w = v4 ? 4 : 1;
  const long long work = (long long)ov.rows * (D / w) + (long long)B * (iov.cols / w);
  launch_form<Gather>(h->format, v4, work, s, view_of(h), ivv, reinterpret_cast<const int *>(ci->stage.dev), B, first_t, ov, iov);
  TDNNF_LAUNCH_CHECK();
  h->gathers++;
  h->last_form = w;
  return TDNNF_OK;
}

int tdnnf_feature_store_info(const tdnnf_feature_store *h, int *format, int *feat_dim, int *utterances, long long *frames, long long *device_bytes,
                             long long *reserved_bytes, long long *allocations, long long *gathers, long long *expands, int *last_form) {
  TDNNF_REQUIRE(h, "feature_store_info: null handle");
  if (format) *format = h->format;
  if (feat_dim) *feat_dim = h->feat_dim;
  if (utterances) *utterances = (int)h->frames.size();
  if (frames) *frames = h->total_frames;
  if (device_bytes) *device_bytes = h->code_bytes + (long long)h->frames.size() * utt_side_bytes(h->format, h->feat_dim);
  if (reserved_bytes) *reserved_bytes = (long long)h->stage.arena_bytes;
  if (allocations) *allocations = h->stage.device_allocs + h->stage.pinned_allocs - h->allocs_at_create;
  if (gathers) *gathers = h->gathers;
  if (expands) *expands = h->expands;
  if (last_form) *last_form = h->last_form;
  return TDNNF_OK;
}

int tdnnf_feature_store_frames(const tdnnf_feature_store *h, int first, int count, int *frames_out) {
  TDNNF_REQUIRE(h && frames_out && first >= 0 && count >= 0 && (long long)first + count <= (long long)h->frames.size(),
                "feature_store_frames: utterances [%d, %d + %d) of %d", first, first, count, h ? (int)h->frames.size() : 0);
  for (int i = 0; i < count; i++) frames_out[i] = h->frames[first + i];
  return TDNNF_OK;
}

}  // extern "C"
