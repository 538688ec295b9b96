// align_build_kernels.h -- the device build of a reserved tdnnf_align_graphs (align_build.hip launches it, tdnnf_align_graphs_assign asks for it):
// from the staged raw arrays of a batch the tables of align_tables.h, byte for byte what align_build_tables(..., columns = true, arc_label)
// gives on the host.  Three launches, the cross-graph offsets going through the kernel boundaries:
//   align_build_rows_kernel     grid (graphs, tables): one workgroup sizes one graph's share of one table -- the length of every row, every
//                               arc's place in its row, the rows' order (light rows by descending length, stable; heavy rows behind them in
//                               row order), the first entry of every slice and heavy row LOCAL to the graph, and the graph's three counts;
//   align_build_offsets_kernel  grid (tables): the exclusive sums of the counts over the graphs, the AlignGraphDev ranges, the totals;
//   align_build_fill_kernel     grid (graphs, tables, parts): slots, heavy-row descriptors, the padding of the slices and the arcs.
// Everything is in global memory (the handle's scratch, AlignBuildTable), so a graph may be as large as a denominator graph; LDS holds only a
// chunk's keys, a scan and 66 counters.  No atomics at all: an arc's place in its row, and a row's place among the rows of its length, is
// the count of earlier entries with the same key -- per chunk of kBuildThreads entries the count of lower threads with the key (a loop over
// the chunk's keys in LDS) on top of a running counter per key, which the chunk's last thread with that key moves on.  Each such counter
// has one writer per chunk, and workgroup barriers order the chunks (build_stable_place and build_scan: build_place.h, shared with the
// supervision's build); no workgroup waits on another; every loop's count is known at its start.
#pragma once
#include "align_graphs.h"
#include "build_place.h"

namespace tdnnf {
namespace {

constexpr int kBuildBuckets = kAlignHeavy + 2;  // a light row of length l: bucket kAlignHeavy - l (descending length); heavy rows: the last

// the first index in list[0 .. n) that is not below v (v is in the list: the rank of a pdf or label in its graph's column list)
__device__ inline int build_rank(const int *list, int n, int v) {
  int lo = 0, hi = n;
  while (lo < hi) {  // (at most 31 halvings of n)
    const int mid = (lo + hi) >> 1;
    if (list[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

struct BuildGraph {  // graph k's share of table t
  int s0, a0, a1;    // its first state, its arcs
  int rowbase, R;    // its rows in the table's per-row scratch
  const int *cols;   // by_pdf / by_label: its column list
};

__device__ inline BuildGraph build_graph(const AlignBuildDev &b, int t, int k) {
  BuildGraph g;
  g.s0 = b.state_begin[k];
  g.a0 = b.arc_begin[k];
  g.a1 = b.arc_begin[k + 1];
  g.cols = nullptr;
  if (t < 2) {
    g.rowbase = g.s0;
    g.R = b.state_begin[k + 1] - g.s0;
  } else if (t == 2) {
    g.rowbase = b.col_begin[k];
    g.R = b.col_begin[k + 1] - g.rowbase;
    g.cols = b.col_pdfs + g.rowbase;
  } else {
    g.rowbase = b.lcol_begin[k];
    g.R = b.lcol_begin[k + 1] - g.rowbase;
    g.cols = b.col_labels + g.rowbase;
  }
  return g;
}

// the row of arc a, local to its graph
__device__ inline int build_row(const AlignBuildDev &b, int t, const BuildGraph &g, int a) {
  if (t == 0) return b.dst[a] - g.s0;
  if (t == 1) return b.src[a] - g.s0;
  return build_rank(g.cols, g.R, t == 2 ? b.pdf[a] : b.label[a]);
}

__device__ inline int build_bucket(int len) { return len > kAlignHeavy ? kAlignHeavy + 1 : kAlignHeavy - len; }

__global__ __launch_bounds__(kBuildThreads) void align_build_rows_kernel(AlignBuildDev b) {
  __shared__ int keys[kBuildThreads];
  __shared__ int hist[kBuildBuckets], start[kBuildBuckets];
  __shared__ int carry;
  const int k = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
  const AlignBuildTable &T = b.t[t];
  const BuildGraph g = build_graph(b, t, k);
  int *len = T.len + g.rowbase, *order = T.order + g.rowbase, *rowpos = T.rowpos + g.rowbase, *off = T.off + g.rowbase;

  // the rows' lengths and every arc's place in its row
  for (int r = tid; r < g.R; r += kBuildThreads) len[r] = 0;
  __syncthreads();
  const int A = g.a1 - g.a0;
  for (int base = 0; base < A; base += kBuildThreads) {
    const int a = g.a0 + base + tid;
    const bool valid = base + tid < A;
    const int row = valid ? build_row(b, t, g, a) : 0;
    const int place = build_stable_place(row, valid, keys, len);
    if (valid) T.arcpos[a] = place;
  }

  // the rows' order: a stable counting sort by bucket
  for (int i = tid; i < kBuildBuckets; i += kBuildThreads) hist[i] = 0;
  __syncthreads();
  for (int base = 0; base < g.R; base += kBuildThreads) {
    const int r = base + tid;
    const bool valid = r < g.R;
    const int place = build_stable_place(valid ? build_bucket(len[r]) : 0, valid, keys, hist);
    if (valid) rowpos[r] = place;
  }
  if (tid == 0) {
    int sum = 0;
    for (int i = 0; i < kBuildBuckets; i++) {
      start[i] = sum;
      sum += hist[i];
    }
  }
  __syncthreads();
  const int nl = start[kBuildBuckets - 1], nh = hist[kBuildBuckets - 1], nslices = (nl + 63) / 64;
  for (int r = tid; r < g.R; r += kBuildThreads) {
    const int q = start[build_bucket(len[r])] + rowpos[r];
    rowpos[r] = q;
    if (q >= 0 && q < g.R) order[q] = r;  // (always: the buckets' counts sum to R)
  }
  if (tid == 0) carry = 0;
  __syncthreads();

  // the first entry of every slice (64 lanes of its first row's length), then of every heavy row
  for (int base = 0; base < nslices; base += kBuildThreads) {
    const int i = base + tid;
    const int before = build_scan(i < nslices ? 64 * len[order[64 * i]] : 0, keys, &carry);
    if (i < nslices) off[i] = before;
  }
  for (int base = 0; base < nh; base += kBuildThreads) {
    const int h = base + tid;
    const int before = build_scan(h < nh ? len[order[nl + h]] : 0, keys, &carry);
    if (h < nh) off[nslices + h] = before;
  }
  if (tid == 0) T.ginfo[k] = make_int4(64 * nslices, nh, carry, nl);
}

__global__ __launch_bounds__(kBuildThreads) void align_build_offsets_kernel(AlignBuildDev b) {
  __shared__ int scan[kBuildThreads];
  __shared__ int carry[3];
  const int t = blockIdx.x, tid = threadIdx.x;
  const AlignBuildTable &T = b.t[t];
  if (tid < 3) carry[tid] = 0;
  __syncthreads();
  for (int base = 0; base < b.G; base += kBuildThreads) {
    const int k = base + tid;
    const bool valid = k < b.G;
    const int4 n = valid ? T.ginfo[k] : make_int4(0, 0, 0, 0);
    const int slot0 = build_scan(n.x, scan, &carry[0]);
    const int heavy0 = build_scan(n.y, scan, &carry[1]);
    const int arc0 = build_scan(n.z, scan, &carry[2]);
    if (!valid) continue;
    T.gbase[k] = make_int4(slot0, heavy0, arc0, 0);
    const AlignRange range = {slot0, n.x, heavy0, n.y};
    if (t == 0) {
      b.graphs[k].state0 = b.state_begin[k];
      b.graphs[k].num_states = b.state_begin[k + 1] - b.state_begin[k];
      b.graphs[k].by_dst = range;
    } else if (t == 1) {
      b.graphs[k].by_src = range;
    } else if (t == 2) {
      b.graphs[k].by_pdf = range;
    } else {
      b.label_range[k] = range;
    }
  }
  if (tid < 3) T.totals[tid] = carry[tid];
}

__global__ __launch_bounds__(kBuildThreads) void align_build_fill_kernel(AlignBuildDev b) {
  const int k = blockIdx.x, t = blockIdx.y;
  const int first = blockIdx.z * kBuildThreads + threadIdx.x, step = gridDim.z * kBuildThreads;
  const AlignBuildTable &T = b.t[t];
  const BuildGraph g = build_graph(b, t, k);
  const int *len = T.len + g.rowbase, *order = T.order + g.rowbase, *rowpos = T.rowpos + g.rowbase, *off = T.off + g.rowbase;
  const int4 n = T.ginfo[k], at = T.gbase[k];
  const int num_slots = n.x, nh = n.y, nl = n.w, nslices = num_slots / 64;

  // the slots and the padding of their lanes
  for (int q = first; q < num_slots; q += step) {
    const int r = q < nl ? order[q] : -1, l = q < nl ? len[r] : 0;
    const int lane0 = at.z + off[q >> 6] + (q & 63), width = len[order[q & ~63]];
    if (at.x + q < T.cap_slots)
      T.slots[at.x + q] = q < nl ? make_int4(t == 2 ? g.cols[r] : r, l, lane0, t >= 2 ? r : 0) : make_int4(-1, 0, 0, 0);
    for (int j = l; j < width; j++)
      if (lane0 + 64 * j < T.cap_arcs) T.arcs[lane0 + 64 * j] = make_int4(0, 0, 0, -1);
  }
  for (int h = first; h < nh; h += step) {
    const int r = order[nl + h], begin = at.z + off[nslices + h];
    if (at.y + h < T.cap_heavy) T.heavy[at.y + h] = make_int4(t == 2 ? g.cols[r] : r, begin, begin + len[r], t >= 2 ? r : 0);
  }
  // the arcs, each to its place in its row
  for (int a = g.a0 + first; a < g.a1; a += step) {
    const int r = build_row(b, t, g, a), q = rowpos[r], j = T.arcpos[a];
    const int e = at.z + (len[r] <= kAlignHeavy ? off[q >> 6] + 64 * j + (q & 63) : off[nslices + q - nl] + j);
    const int src = b.src[a] - g.s0, dst = b.dst[a] - g.s0, pdf = b.pdf[a], lp = b.lp_bits[a];
    const int4 v = t == 0 ? make_int4(src, pdf, lp, a) : t == 1 ? make_int4(dst, pdf, lp, a) : t == 2 ? make_int4(src, dst, lp, a) : make_int4(src, dst, lp, pdf);
    if (e >= 0 && e < T.cap_arcs) T.arcs[e] = v;
  }
}

}  // namespace
}  // namespace tdnnf
