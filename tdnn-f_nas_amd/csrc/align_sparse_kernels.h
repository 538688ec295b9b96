// align_sparse_kernels.h -- the selection pass of the sparse posteriors (include/tdnnf_hip.h, "sparse posteriors"): from the compact block
// of a forward-backward call (align_fb_kernels.h: per utterance frames x D floats, column k = pdf pdfs_g[k], ascending) to at most K
// (pdf, value) pairs a frame.  Included by align_sparse.hip.
//
// Per frame, with v[k] the row's floats:
//     candidates   the columns with v[k] > min_post (strict; min_post >= 0, so a zero, a negative value and a NaN never are), n of them;
//     kept         all of them if n <= K, else the K of greatest value, among equal values the lower pdf;
//     written      in ascending pdf order to slots [f * K, f * K + count), count = min(n, K); slots [count, K) get (-1, 0.f).
// Nothing is computed: the values are the compact block's bits, so the pass is as deterministic as its input.
//
// align_sparse_select_kernel: a wave per frame, kAlignSparseWaves waves a workgroup, each taking kAlignSparseFrames frames in turn; grid
// (frame groups, utterances).  The lanes stride the row in ascending column order, so a 64-bit ballot of "kept" and a popcount of the
// lower lanes give a kept column its position among the kept ones: one owner per slot, no atomics, no list of candidates anywhere.
//   1. one sweep counts n;
//   2. n > K: the cutoff c, the K-th greatest candidate.  Candidates are positive floats, which order as their bit patterns taken as
//      unsigned integers, so c is built from bit 30 down: a bit stays set if at least K candidates are >= the pattern so far -- a sweep
//      with one ballot a stride per bit.  Kept: everything above c and the first K - |above c| columns equal to c.  As soon as EXACTLY
//      K candidates are >= the pattern so far they are the kept ones and the search ends: about log2(n / K) + 2 sweeps where the values
//      differ, all 31 and one more only where several columns hold the cutoff's value;
//   3. one sweep writes the kept pairs.
// The sweeps after the first re-read the row (D floats: 1.2 KB on a transcript graph, 24 KB at 6 030 columns) from the caches.  Step 2 is
// the slow path: with a floor that means something, few frames have more than K candidates.
// A workgroup leaves (frames with n > K, greatest n) of its frames in `parts`; align_sparse_results_kernel folds them per utterance.
#pragma once
#include "align_graphs.h"

namespace tdnnf {
namespace {

constexpr int kAlignSparseWaves = 4;   // waves a workgroup
constexpr int kAlignSparseFrames = 4;  // frames a wave
constexpr int kAlignSparseGroup = kAlignSparseWaves * kAlignSparseFrames;  // frames a workgroup
constexpr int kAlignSparseMaxK = 64;   // one lane per slot of a frame

struct AlignSparseUtt {   // one utterance of a call (device table in the workspace)
  long long block_begin;  // first float of its block in the compact block
  int frames;
  int frame_begin;        // its first frame among the call's: the exclusive prefix sum of utt_frames
  int D;                  // columns of its graph
  int col_begin;          // the graph's column list starts here in tdnnf_align_graphs::col_pdfs_dev
  int part_begin;         // its first workgroup's pair in parts; it has ceil(frames / kAlignSparseGroup) of them
  int pad;
};

static_assert(sizeof(AlignSparseUtt) == 32, "the workspace formula of include/tdnnf_hip.h counts 32 bytes an utterance");

// candidates of the row whose pattern is at least `least` (least > 0: a column that is no candidate enters as 0); the same in every lane
__device__ __forceinline__ int align_sparse_count(const float *v, int D, float min_post, unsigned least) {
  const int lane = threadIdx.x & 63;
  int n = 0;
  for (int base = 0; base < D; base += 64) {
    const int k = base + lane;
    const float x = k < D ? v[k] : 0.f;
    const unsigned bits = x > min_post ? __float_as_uint(x) : 0u;
    n += __popcll(__ballot(bits >= least));
  }
  return n;
}

// grid (ceil(max frames / kAlignSparseGroup), utterances), kAlignSparseWaves * 64 threads.  1 <= K <= kAlignSparseMaxK.
__global__ __launch_bounds__(kAlignSparseWaves * 64) void align_sparse_select_kernel(const AlignSparseUtt *utts, const float *compact, const int *col_pdfs,
                                                                                     float min_post, int K, int *pdf_out, float *post_out,
                                                                                     int *count_out, int2 *parts) {
  __shared__ int2 wave_part[kAlignSparseWaves];
  const AlignSparseUtt u = utts[blockIdx.y];
  const int t0 = blockIdx.x * kAlignSparseGroup;
  if (t0 >= u.frames) return;  // (the whole workgroup: the grid covers the call's longest utterance)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1;
  const int *pdfs = col_pdfs + u.col_begin;
  const int D = u.D;
  int truncated = 0, most = 0;
  for (int i = 0; i < kAlignSparseFrames; i++) {
    const int t = t0 + i * kAlignSparseWaves + wave;
    if (t >= u.frames) break;  // (the wave's later frames lie further still)
    const float *v = compact + u.block_begin + (size_t)t * D;
    const size_t slot0 = (size_t)(u.frame_begin + t) * K;
    const int n = align_sparse_count(v, D, min_post, 1u);
    most = max(most, n);
    // kept: the candidates whose pattern is at least all_from, and the first `ties` columns whose pattern is cut
    unsigned all_from = 1u, cut = 0;
    int ties = 0;
    if (n > K) {
      truncated++;
      all_from = 0;
      for (unsigned bit = 1u << 30; bit && !all_from; bit >>= 1) {
        const int c = align_sparse_count(v, D, min_post, cut | bit);
        if (c >= K) cut |= bit;
        if (c == K) all_from = cut;  // exactly K candidates from here up: no tie to break, the lower bits do not matter
      }
      if (!all_from) {  // cut is the K-th greatest value and more than K candidates are >= cut: several columns hold it
        all_from = cut + 1;  // (cut < 2^31: a candidate's sign bit is clear)
        ties = K - align_sparse_count(v, D, min_post, all_from);
      }
    }
    int kept = 0, equal = 0;
    for (int base = 0; base < D; base += 64) {
      const int k = base + lane;
      const float x = k < D ? v[k] : 0.f;
      const unsigned bits = x > min_post ? __float_as_uint(x) : 0u;
      const unsigned long long eq = __ballot(bits == cut);  // (cut 0, no truncation: counted, never asked for)
      const bool keep = bits >= all_from || (bits == cut && equal + __popcll(eq & below) < ties);
      const unsigned long long km = __ballot(keep);
      if (keep) {
        const int pos = kept + __popcll(km & below);  // < min(n, K)
        pdf_out[slot0 + pos] = pdfs[k];
        post_out[slot0 + pos] = x;
      }
      kept += __popcll(km);
      equal += __popcll(eq);
    }
    if (lane >= kept && lane < K) {
      pdf_out[slot0 + lane] = -1;
      post_out[slot0 + lane] = 0.f;
    }
    if (lane == 0) count_out[u.frame_begin + t] = kept;
  }
  if (lane == 0) wave_part[wave] = make_int2(truncated, most);
  __syncthreads();
  if (threadIdx.x == 0) {
    int2 p = wave_part[0];
    for (int w = 1; w < kAlignSparseWaves; w++) {
      p.x += wave_part[w].x;
      p.y = max(p.y, wave_part[w].y);
    }
    parts[u.part_begin + blockIdx.x] = p;
  }
}

// grid utterances, 64 threads: results[4 u ..] = (logprob, ok) of the compact call's fb_results, the utterance's frames with n > K and its
// greatest n -- integers, so the order of the fold is no matter
__global__ __launch_bounds__(64) void align_sparse_results_kernel(const AlignSparseUtt *utts, const double *fb_results, const int2 *parts, double *results) {
  const AlignSparseUtt u = utts[blockIdx.x];
  const int lane = threadIdx.x, num = (u.frames + kAlignSparseGroup - 1) / kAlignSparseGroup;
  int truncated = 0, most = 0;
  for (int i = lane; i < num; i += 64) {
    const int2 p = parts[u.part_begin + i];
    truncated += p.x;
    most = max(most, p.y);
  }
  for (int o = 32; o > 0; o >>= 1) {
    truncated += __shfl_xor(truncated, o, 64);
    most = max(most, __shfl_xor(most, o, 64));
  }
  if (lane == 0) {
    double *r = results + 4 * (size_t)blockIdx.x;
    r[0] = fb_results[2 * (size_t)blockIdx.x];
    r[1] = fb_results[2 * (size_t)blockIdx.x + 1];
    r[2] = (double)truncated;
    r[3] = (double)most;
  }
}

}  // namespace
}  // namespace tdnnf
