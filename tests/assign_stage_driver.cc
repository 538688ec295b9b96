// assign_stage_driver.cc -- the plain half of tdnn-f_nas_amd/csrc/assign_stage.h (the packing of a batch's arrays into a staging buffer, the
// carve, the capacity refusal: what runs on the host before anything reaches the device) as a stand-alone program, for a build under the
// address and undefined-behaviour sanitizers.  The buffers are heap blocks of exactly the size the packer is told, so an append that
// wrote beyond it would be reported.  It prints the layout of one small labelled batch, packed in tdnnf_align_graphs_assign's order, for
// tests/test_assign_stage_cpu.py to hold against the layout written down there.  No device, no library.
// Build: g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I tdnn-f_nas_amd/csrc tests/assign_stage_driver.cc
#include <cstdio>
#include <cstring>
#include <vector>

#include "assign_stage.h"

using namespace tdnnf;

static int failures = 0;
#define EXPECT(cond, ...)          \
  do {                             \
    if (!(cond)) {                 \
      std::printf("FAILED %s: ", #cond); \
      std::printf(__VA_ARGS__);    \
      std::printf("\n");           \
      failures++;                  \
    }                              \
  } while (0)

static void offsets() {
  std::vector<char> buf(40, 'x');
  const int a[3] = {1, 2, 3}, b[2] = {4, 5};
  const float c[4] = {0.5f, -1.f, 2.f, 8.f};
  int dst_b, dst_c, dst_none;
  StagePacker p{buf.data(), buf.size()};
  // raw entries in front of direct ones, one behind the other; an empty array takes no bytes and no copy entry
  EXPECT(p.put(a, 3) == 0 && p.at == 12, "%zu", p.at);
  EXPECT(p.put(nullptr, 0) == 12 && p.at == 12, "%zu", p.at);
  EXPECT(p.put(c, 4) == 12 && p.at == 28, "%zu", p.at);
  const size_t raw_bytes = p.at;
  EXPECT(p.put_to(&dst_none, nullptr, 0) == 28 && p.at == 28 && p.num_copies == 0, "%zu %d", p.at, p.num_copies);
  EXPECT(p.put_to(&dst_b, b, 2) == 28 && p.at == 36 && p.num_copies == 1, "%zu %d", p.at, p.num_copies);
  EXPECT(p.put_to(&dst_c, c, 1) == 36 && p.at == 40 && p.num_copies == 2 && p.fits(), "%zu %d", p.at, p.num_copies);
  EXPECT(p.copies[0].to == &dst_b && p.copies[0].from == 28 && p.copies[0].bytes == 8, "%zu %zu", p.copies[0].from, p.copies[0].bytes);
  EXPECT(p.copies[1].to == &dst_c && p.copies[1].from == 36 && p.copies[1].bytes == 4, "%zu %zu", p.copies[1].from, p.copies[1].bytes);
  for (int i = 0; i < p.num_copies; i++) EXPECT(p.copies[i].from >= raw_bytes, "copy %d starts inside the raw prefix", i);
  EXPECT(!std::memcmp(buf.data(), a, 12) && !std::memcmp(buf.data() + 12, c, 16) && !std::memcmp(buf.data() + 28, b, 8) && !std::memcmp(buf.data() + 36, c, 4),
         "the buffer does not hold the arrays one behind the other");
  std::printf("offsets: %zu raw bytes, %zu in all, %d copies\n", raw_bytes, p.at, p.num_copies);
}

static void refusals() {
  std::vector<char> buf(20, 'x');
  const int a[4] = {1, 2, 3, 4};
  int dst;
  StagePacker p{buf.data(), buf.size()};
  EXPECT(p.put(a, 4) == 0 && p.fits(), "%zu", p.at);
  // 8 bytes into the 4 that are left: refused, nothing written, no copy entry; `at` says what the batch needed
  EXPECT(p.put_to(&dst, a, 2) == 16 && !p.fits() && p.at == 24 && p.num_copies == 0, "%zu %d", p.at, p.num_copies);
  EXPECT(buf[16] == 'x' && buf[19] == 'x', "the refused append wrote");
  // ... and what would fit behind a refused append is refused as well: the offsets are no longer the device staging's
  EXPECT(p.put(a, 1) == 24 && !p.fits() && p.at == 28 && buf[16] == 'x', "%zu", p.at);
  std::printf("refusal: needs %zu bytes of %zu\n", p.at, p.size);

  // an append that ends exactly at the size fits
  StagePacker q{buf.data(), buf.size()};
  EXPECT(q.put(a, 4) == 0 && q.put_to(&dst, a, 1) == 16 && q.fits() && q.at == 20 && q.num_copies == 1, "%zu", q.at);

  // the copy list at its capacity: the next entry is refused, nothing written, nothing beyond the list touched
  std::vector<char> big(4 * (StagePacker::kMaxCopies + 2), 'x');
  StagePacker r{big.data(), big.size()};
  for (int i = 0; i < StagePacker::kMaxCopies; i++) r.put_to(&dst, a, 1);
  EXPECT(r.fits() && r.num_copies == StagePacker::kMaxCopies && r.at == 4 * (size_t)StagePacker::kMaxCopies, "%zu %d", r.at, r.num_copies);
  r.put_to(&dst, a, 1);
  EXPECT(!r.fits() && r.list_full && r.num_copies == StagePacker::kMaxCopies && big[4 * StagePacker::kMaxCopies] == 'x', "%d", r.num_copies);
  r.put_to(&dst, nullptr, 0);  // (an empty array asks for no entry)
  EXPECT(r.num_copies == StagePacker::kMaxCopies, "%d", r.num_copies);
  std::printf("refusal: copy list full at %d\n", r.num_copies);
}

// A labelled batch of 2 graphs, 5 states and 7 arcs between them (graph 0: 2 states, 3 arcs on pdfs {4, 9} with labels {0, 1}; graph 1:
// 3 states, 4 arcs on pdfs {1, 4, 6} with labels {0, 2}), packed in the order of tdnnf_align_graphs_assign (align_graphs.hip).
static void align_batch() {
  const int G = 2, NS = 5, NA = 7;
  const int state_begin[3] = {0, 2, 5}, arc_begin[3] = {0, 3, 7};
  const int src[7] = {0, 0, 1, 2, 2, 3, 4}, dst[7] = {0, 1, 1, 3, 2, 4, 4}, pdf[7] = {4, 9, 4, 1, 6, 4, 1}, label[7] = {0, 1, 1, 0, 0, 2, 2};
  const float lp[7] = {-1, -2, -3, -4, -5, -6, -7}, init[5] = {0, -9, 0, -9, -9}, fin[5] = {-9, 0, -9, -9, 0};
  const int col_begin[3] = {0, 2, 5}, col_pdfs[5] = {4, 9, 1, 4, 6}, num_cols[2] = {2, 3};
  const int lcol_begin[3] = {0, 2, 4}, col_labels[4] = {0, 1, 0, 2}, num_lcols[2] = {2, 2};
  int handle[7];  // (stand-ins for the handle's device arrays)
  std::vector<char> buf(sizeof(int) * (4 * (G + 1) + 7 * NA + 2 * NS + 2 * G));  // what tdnnf_align_graphs_reserve sizes for these capacities
  StagePacker p{buf.data(), buf.size()};
  std::printf("layout:");
  const auto show = [&](size_t begin) { std::printf(" %zu %zu", begin, p.at - begin); };
  show(p.put(state_begin, G + 1));
  show(p.put(arc_begin, G + 1));
  show(p.put(col_begin, G + 1));
  show(p.put(lcol_begin, G + 1));
  show(p.put(src, NA));
  show(p.put(dst, NA));
  show(p.put(pdf, NA));
  show(p.put(lp, NA));
  std::printf(" raw %zu", p.at);
  show(p.put_to(&handle[0], init, NS));
  show(p.put_to(&handle[1], fin, NS));
  show(p.put_to(&handle[2], num_cols, G));
  show(p.put_to(&handle[3], col_pdfs, 5));
  show(p.put_to(&handle[4], label, NA));
  show(p.put_to(&handle[5], num_lcols, G));
  show(p.put_to(&handle[6], col_labels, 4));
  std::printf(" copies %d of %zu\n", p.num_copies, buf.size());
  EXPECT(p.fits() && p.num_copies == 7, "%zu %d", p.at, p.num_copies);
  for (int i = 0; i < p.num_copies; i++) EXPECT(p.copies[i].to == &handle[i], "copy %d", i);
  EXPECT(!std::memcmp(buf.data() + p.copies[4].from, label, sizeof(label)) && !std::memcmp(buf.data() + 132, lp, sizeof(lp)), "the buffer's bytes");
}

static void carve_and_capacity() {
  Carve size{nullptr, 0};
  EXPECT(size.take<int>(3) == nullptr && size.at == 12, "%zu", size.at);
  EXPECT(size.take<char>(0) == nullptr && size.at == 257, "%zu", size.at);  // (a piece of one element at least, 256 bytes on)
  EXPECT(size.take<double>(2) == nullptr && size.at == 528, "%zu", size.at);
  std::vector<char> block(size.at);
  Carve c{block.data(), 0};
  EXPECT((char *)c.take<int>(3) == block.data() && c.take<char>(0) == block.data() + 256 && (char *)c.take<double>(2) == block.data() + 512 && c.at == size.at,
         "%zu", c.at);
  std::string err;
  EXPECT(within_capacity("driver: ", 7, "arcs", 7, &err) && err.empty(), "%s", err.c_str());
  EXPECT(!within_capacity("driver: ", 9, "arcs", 7, &err) && err == "driver: 9 arcs exceed the capacity max_arcs = 7 by 2", "%s", err.c_str());
  std::printf("capacity: %s\n", err.c_str());
}

int main() {
  offsets();
  refusals();
  align_batch();
  carve_and_capacity();
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
