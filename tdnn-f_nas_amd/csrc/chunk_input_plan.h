// chunk_input_plan.h -- the host half of the chunk minibatch inputs (include/tdnnf_hip.h, "CHUNK INPUTS"; chunk_input.hip): the checks of a
// minibatch of chunks against the stacked utterances and the table the gather kernel reads, 4 ints a sequence.  One function serves
// tdnnf_chunk_input_plan and tdnnf_chunk_input_gather, so what the one reports is what the other stages.  Plain C++ with no device header:
// tests/chunk_input_driver.cc builds it with g++ under the sanitizers.
#pragma once
#include <stdio.h>

#include <string>
#include <vector>

namespace tdnnf {

constexpr int kChunkTab = 4;  // per sequence: [first stacked feature row of the utterance, frames[u], begin * fsf - frame_shift, stacked i-vector row]

// The stacked rows the minibatch's utterances take: what feats and ivectors must have.
struct ChunkInputRows {
  long long feat_rows, ivector_rows;
};

namespace chunk_input_detail {
inline bool refuse(std::string *err, const char *who, const char *fmt, long long a = 0, long long b = 0, long long c = 0, long long d = 0) {
  char buf[512], msg[400];
  snprintf(msg, sizeof(msg), fmt, a, b, c, d);
  snprintf(buf, sizeof(buf), "%s%s", who, msg);
  *err = buf;
  return false;
}
}  // namespace chunk_input_detail

// Validates a minibatch of B chunks of T output frames and writes its table (kChunkTab * B ints; table may be null: the checks alone).
// use_iv: i-vectors are gathered -- iv_rows (period > 0) is read and every R_u must be >= 1, entry 3 is the stacked row of "CHUNK INPUTS";
// else entry 3 is 0 and iv_rows is not read.  false with *err naming the offending sequence or utterance; nothing is written then.
inline bool chunk_input_plan(const char *who, int fsf, int T, int B, const int *seq_utt, const int *chunk_begin, int frame_shift, int U, const int *frames,
                             bool use_iv, const int *iv_rows, int period, int *table, ChunkInputRows *rows, std::string *err) {
  using chunk_input_detail::refuse;
  if (fsf < 1 || T < 1) return refuse(err, who, "frame_subsampling %lld and frames_per_sequence %lld must be positive", fsf, T);
  if (B < 1 || !seq_utt || !chunk_begin) return refuse(err, who, "%lld sequences: seq_utt_host and chunk_begin_host must hold one entry a sequence, at least one", B);
  if (U < 1 || !frames) return refuse(err, who, "%lld utterances: frames_host must hold one length an utterance, at least one", U);
  if (frame_shift <= -fsf || frame_shift >= fsf)
    return refuse(err, who, "frame_shift %lld: its magnitude must be below frame_subsampling %lld", frame_shift, fsf);
  const bool counted = use_iv && period > 0;
  if (counted && !iv_rows) return refuse(err, who, "ivector_period %lld > 0 needs ivector_rows_host", period);
  long long sumT = 0, sumR = 0;
  std::vector<long long> feat0(U), iv0(U);  // the first stacked rows of every utterance
  for (int u = 0; u < U; u++) {
    feat0[u] = sumT;
    iv0[u] = sumR;
    if (frames[u] < 1) return refuse(err, who, "utterance %lld has %lld frames", u, frames[u]);
    if (counted && iv_rows[u] < 1) return refuse(err, who, "utterance %lld has no i-vector rows (%lld)", u, iv_rows[u]);
    sumT += frames[u];
    sumR += use_iv ? (counted ? iv_rows[u] : 1) : 0;
  }
  if (sumT + 2LL * fsf >= (1LL << 31) || sumR >= (1LL << 31)) return refuse(err, who, "too many stacked rows (%lld of features, %lld of i-vectors)", sumT, sumR);
  for (int b = 0; b < B; b++) {
    const int u = seq_utt[b];
    if (u < 0 || u >= U) return refuse(err, who, "sequence %lld: utterance %lld outside [0, %lld)", b, u, U);
    const long long O = ((long long)frames[u] + fsf - 1) / fsf, o = chunk_begin[b];
    if (o < 0) return refuse(err, who, "sequence %lld: the chunk begins at frame %lld", b, o);
    if (o + T > O)
      return refuse(err, who, "sequence %lld: the chunk of %lld frames from frame %lld ends behind the %lld output frames of the utterance", b, T, o, O);
  }
  if (rows) *rows = ChunkInputRows{sumT, sumR};
  if (!table) return true;
  // (a second walk: a refusal above has written nothing)
  for (int b = 0; b < B; b++) {
    const int u = seq_utt[b];
    int *t = table + kChunkTab * b;
    t[0] = (int)feat0[u];
    t[1] = frames[u];
    t[2] = (int)((long long)chunk_begin[b] * fsf - frame_shift);
    long long row = 0;
    if (counted) {
      row = ((long long)chunk_begin[b] + T / 2) * fsf / period;
      if (row > iv_rows[u] - 1) row = iv_rows[u] - 1;
    }
    t[3] = use_iv ? (int)(iv0[u] + row) : 0;
  }
  return true;
}

}  // namespace tdnnf
