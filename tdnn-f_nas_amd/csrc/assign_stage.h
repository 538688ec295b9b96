// assign_stage.h -- what the handles that are allocated once and assigned a batch per call in stream order share (align_graphs.hip,
// chain_sup_build.hip; DESIGN.md "One staging for the assigns"): the carve of the one device allocation, the capacity refusal, the packing of a
// batch's arrays into a staging buffer, and the two pinned staging buffers that take turns.  An assign: its checks (a refusal leaves all
// as it was), AssignStage::begin, put / put_to, the handle's count of assigns to 0, AssignStage::submit, the build's launches, the commit with
// the count at what it was plus one -- so from the first enqueued copy until success the handle holds no batch and every reader refuses it.
// The first half is plain C++ with no device header: tests/assign_stage_driver.cc builds it with g++ under the sanitizers.
#pragma once
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>

namespace tdnnf {

// A batch against one capacity; false with *err naming the capacity, its value and the excess.  who: the prefix of the message, the call's
// name; what: "graphs", "states", "arcs", "sequences", "frames".
inline bool within_capacity(const char *who, int n, const char *what, int capacity, std::string *err) {
  if (n <= capacity) return true;
  char buf[512];
  snprintf(buf, sizeof(buf), "%s%d %s exceed the capacity max_%s = %d by %d", who, n, what, what, capacity, n - capacity);
  *err = buf;
  return false;
}

// Hands out pieces of a handle's one allocation, 256 bytes apart at least and of one element at least; with a null base it only counts.
struct Carve {
  char *base;
  size_t at;
  template <class T>
  T *take(size_t n) {
    at = (at + 255) & ~(size_t)255;
    T *p = base ? reinterpret_cast<T *>(base + at) : nullptr;
    at += sizeof(T) * std::max<size_t>(n, 1);
    return p;
  }
};

// Packs a batch's arrays of 4-byte elements into one staging buffer, one behind the other; an array's offset is the same in the device
// staging.  put: an array the build reads there (the raw prefix: the caller notes `at` behind the last).  put_to: an array that goes to a
// device array of the handle as it is; AssignStage::submit copies each from the buffer.  An append that does not fit the buffer or the copy
// list writes nothing and leaves fits() false; `at` counts on and says what was needed.
struct StagePacker {
  static constexpr int kMaxCopies = 8;
  struct Copy { const void *to; size_t from, bytes; };
  char *host;
  size_t size, at = 0;
  Copy copies[kMaxCopies];
  int num_copies = 0;
  bool list_full = false;

  size_t put(const void *v, size_t n, const void *to = nullptr) {
    const size_t begin = at;
    if (n && to && num_copies == kMaxCopies) list_full = true;
    if (n == 0 || list_full) return begin;
    at += 4 * n;
    if (at > size) return begin;
    memcpy(host + begin, v, 4 * n);
    if (to) copies[num_copies++] = Copy{to, begin, 4 * n};
    return begin;
  }
  size_t put_to(const void *to, const void *v, size_t n) { return put(v, n, to); }
  bool fits() const { return at <= size && !list_full; }
};

}  // namespace tdnnf

#ifdef __HIP__  // (the compiler's own mark of a .hip file: g++ sees the plain half only)
#include "common.h"

namespace tdnnf {

// The one device allocation of a reserved handle, its two pinned staging buffers and the device staging they are copied to.  Turn k uses
// buffer k & 1 and waits for the copies of turn k - 2 out of it: the only wait of an assign.  A turn is taken when submit is reached,
// whether or not the assign fails behind it; a refusal in front of it takes none.
struct AssignStage {
  void *arena;                       // device, owned: every device array of the handle is a piece of it
  size_t arena_bytes;
  char *host[2];                     // pinned, `bytes` each
  hipEvent_t event[2];               // recorded behind the copies out of host[i]
  bool used[2];
  size_t bytes;
  char *dev;                         // a piece of arena: the raw arrays of the batch, packed as in the buffer
  int turn;
  hipStream_t last_stream;           // of the last submit (the dumps wait for it)
  int device_allocs, pinned_allocs;  // allocations made for the handle (the witness that no assign makes one)

  // Every allocation of a zeroed stage: layout(Carve *) names every device array of the handle -- `dev`, `bytes` of it, among them -- and
  // runs twice, with a null base for the size and over the allocation.  On an error destroy() frees what was made.  what: for the message.
  template <class Layout>
  int create(const char *what, size_t stage_bytes, Layout layout) {
    bytes = stage_bytes;
    Carve size{nullptr, 0};
    layout(&size);
    arena_bytes = size.at;
    hipError_t e = hipMalloc(&arena, arena_bytes);
    if (e == hipSuccess) device_allocs++;
    for (int i = 0; i < 2 && e == hipSuccess; i++)
      if ((e = hipHostMalloc((void **)&host[i], std::max<size_t>(bytes, 1), hipHostMallocDefault)) == hipSuccess) {
        pinned_allocs++;
        e = hipEventCreateWithFlags(&event[i], hipEventDisableTiming);
      }
    if (e != hipSuccess) return hip_status(e, what);
    Carve carve{static_cast<char *>(arena), 0};
    layout(&carve);
    return TDNNF_OK;
  }
  void destroy() {  // (once: the handle goes with it)
    (void)hipFree(arena);
    for (int i = 0; i < 2; i++) {
      if (host[i]) (void)hipHostFree(host[i]);
      if (event[i]) (void)hipEventDestroy(event[i]);
    }
  }
  // The buffer of this turn, empty, once the copies of the turn before last have left it.
  int begin(StagePacker *p) {
    if (used[turn & 1]) TDNNF_HIP(hipEventSynchronize(event[turn & 1]));
    p->host = host[turn & 1];
    p->size = bytes;
    return TDNNF_OK;
  }
  // Enqueues on s the copy of the packed buffer's first raw_bytes to the device staging, then the put_to copies, and the event behind them.
  int submit(const StagePacker &p, size_t raw_bytes, hipStream_t s) {
    const int k = turn++ & 1;
    last_stream = s;
    TDNNF_HIP(hipMemcpyAsync(dev, p.host, raw_bytes, hipMemcpyHostToDevice, s));
    for (int i = 0; i < p.num_copies; i++)
      TDNNF_HIP(hipMemcpyAsync(const_cast<void *>(p.copies[i].to), p.host + p.copies[i].from, p.copies[i].bytes, hipMemcpyHostToDevice, s));
    TDNNF_HIP(hipEventRecord(event[k], s));
    used[k] = true;
    return TDNNF_OK;
  }
};

}  // namespace tdnnf
#endif
