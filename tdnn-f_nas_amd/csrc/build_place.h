// build_place.h -- the two workgroup-wide steps that the device builds of arc tables share (align_build_kernels.h: a reserved
// tdnnf_align_graphs; chain_sup_build_kernels.h: a reserved time-synchronous tdnnf_supervision): an entry's place among the earlier entries
// with its key, and an exclusive sum.  No atomics: per chunk of kBuildThreads entries the count of lower threads with the key (a loop over
// the chunk's keys in LDS) on top of a running counter per key, which the chunk's last thread with that key moves on.  Each such counter
// has one writer per chunk, and workgroup barriers order the chunks.
#pragma once
#include <hip/hip_runtime.h>

namespace tdnnf {
namespace {

constexpr int kBuildThreads = 256;

// One chunk of a stable counting pass: this thread's entry has `key` (valid: the thread has an entry).  Returns the number of earlier
// entries with the key -- counter[key] plus the lower threads of the chunk that have it -- and moves counter[key] past the chunk.  keys:
// kBuildThreads ints of LDS.  counter: LDS or this workgroup's global scratch.  Every thread of the workgroup calls it.
__device__ inline int build_stable_place(int key, bool valid, int *keys, int *counter) {
  const int tid = threadIdx.x;
  keys[tid] = valid ? key : -1;
  __syncthreads();
  int lower = 0, all = 0;
  for (int i = 0; i < kBuildThreads; i++) {
    const int same = keys[i] == key ? 1 : 0;
    all += same;
    lower += i < tid ? same : 0;
  }
  const int place = valid ? counter[key] + lower : 0;
  __syncthreads();  // (every read of the counters is done)
  if (valid && lower == all - 1) counter[key] = place + 1;
  __syncthreads();
  return place;
}

// The exclusive sum over the workgroup of v, on top of *carry (LDS), which moves on by the chunk's sum.  scan: kBuildThreads ints of LDS.
__device__ inline int build_scan(int v, int *scan, int *carry) {
  const int tid = threadIdx.x;
  scan[tid] = v;
  __syncthreads();
  for (int d = 1; d < kBuildThreads; d <<= 1) {
    const int add = tid >= d ? scan[tid - d] : 0;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  const int before = *carry + scan[tid] - v;
  __syncthreads();
  if (tid == kBuildThreads - 1) *carry += scan[tid];
  __syncthreads();
  return before;
}

}  // namespace
}  // namespace tdnnf
