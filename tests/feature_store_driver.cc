// feature_store_driver.cc -- the host half of the feature stores (tdnn-f_nas_amd/csrc/feature_store_plan.h over feature_code_value.h: the
// layout, the checks, the packing and the compression, what runs before anything reaches the device) as a stand-alone program, for a build
// under the address and undefined-behaviour sanitizers.  Every array lives in a heap block of exactly its size, so a read or a write
// beyond it would be reported.  It reads the cases tests/test_feature_store_plan_cpu.py writes -- per store a line of scalars, the offsets,
// then per item its header, Kaldi-order codes and the packed arrays of tests/feature_store_ref.py; per float matrix its bits and codes --,
// holds the functions against them, and runs every refusal.  Floats travel as their bit patterns.  No device, no library.
// Build: g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I tdnn-f_nas_amd/csrc tests/feature_store_driver.cc
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <string>
#include <vector>

#include "feature_store_plan.h"

using namespace tdnnf;

static int failures = 0;
#define EXPECT(cond, ...)                \
  do {                                   \
    if (!(cond)) {                       \
      std::printf("FAILED %s: ", #cond); \
      std::printf(__VA_ARGS__);          \
      std::printf("\n");                 \
      failures++;                        \
    }                                    \
  } while (0)

static std::vector<long long> numbers(std::istream &in, size_t n) {
  std::vector<long long> v(n);
  for (long long &x : v) in >> x;
  return v;
}
static float from_bits(long long b) {
  const int32_t i = (int32_t)b;
  float f;
  std::memcpy(&f, &i, 4);
  return f;
}
static int32_t bits_of(float f) {
  int32_t i;
  std::memcpy(&i, &f, 4);
  return i;
}
template <class T>
static std::vector<T> as(const std::vector<long long> &v) {
  std::vector<T> out(v.size());
  for (size_t i = 0; i < v.size(); i++) out[i] = (T)v[i];
  return out;
}

static void store_case(std::istream &in, int index) {
  int fmt, D, U;
  long long device_bytes;
  in >> fmt >> D >> U >> device_bytes;
  const std::vector<long long> want_offsets = numbers(in, U + 1);
  std::vector<int> frames(U);
  const int w = code_width(fmt);
  for (int u = 0; u < U; u++) {
    long long rows, mn, rg;
    in >> rows >> mn >> rg;
    frames[u] = (int)rows;
    const size_t n = (size_t)rows * D;
    std::vector<uint16_t> pct;
    std::vector<int32_t> want_header;
    if (fmt == 1) {
      pct = as<uint16_t>(numbers(in, 4 * (size_t)D));
      want_header = as<int32_t>(numbers(in, 4 * (size_t)D));
    }
    const std::vector<long long> codes = numbers(in, n), want = numbers(in, n);
    // the payload's arrays in blocks of exactly their size, as an archive's reader would hold them
    std::vector<uint8_t> raw(n * w), got(n * w, 0xAB);
    for (size_t i = 0; i < n; i++) {
      if (w == 2) {
        const uint16_t c = (uint16_t)codes[i];
        std::memcpy(&raw[2 * i], &c, 2);
      } else {
        raw[i] = (uint8_t)codes[i];
      }
    }
    const FeaturePayload p{fmt, from_bits(mn), from_bits(rg), (int)rows, D, fmt == 1 ? pct.data() : nullptr, raw.data()};
    std::string err;
    EXPECT(feature_payload_check("driver: ", u, fmt, D, p, &err) && err.empty(), "store %d item %d: %s", index, u, err.c_str());
    std::vector<float> header(fmt == 1 ? 4 * (size_t)D : 0);
    feature_payload_pack(p, header.data(), got.data());
    for (size_t i = 0; i < n; i++) {
      long long c = got[i];
      if (w == 2) {
        uint16_t c16;
        std::memcpy(&c16, &got[2 * i], 2);
        c = c16;
      }
      if (c != want[i]) {
        EXPECT(c == want[i], "store %d item %d code %zu: %lld, not %lld", index, u, i, c, want[i]);
        break;
      }
    }
    for (size_t i = 0; i < header.size(); i++)
      if (bits_of(header[i]) != want_header[i]) {
        EXPECT(bits_of(header[i]) == want_header[i], "store %d item %d header %zu", index, u, i);
        break;
      }
  }
  std::vector<long long> offsets(U + 1, -7);
  long long total = -7;
  std::string err;
  EXPECT(feature_store_layout("driver: ", fmt, D, U, frames.data(), offsets.data(), &total, &err), "store %d: %s", index, err.c_str());
  EXPECT(offsets == want_offsets && total == device_bytes, "store %d: the layout differs (%lld, not %lld bytes)", index, total, device_bytes);
  for (long long o : offsets) EXPECT(o % 16 == 0, "store %d: offset %lld", index, o);
}

static void float_case(std::istream &in, int index) {
  int fmt, rows, cols;
  long long mn_bits, rg_bits;
  in >> fmt >> rows >> cols >> mn_bits >> rg_bits;
  const size_t n = (size_t)rows * cols;
  const std::vector<long long> x_bits = numbers(in, n), want = numbers(in, n);
  std::vector<float> x(n);
  for (size_t i = 0; i < n; i++) x[i] = from_bits(x_bits[i]);
  float mn = 0, rg = 0;
  std::string err;
  EXPECT(feature_compress_check("driver: ", index, fmt, rows, cols, x.data(), &mn, &rg, &err), "float %d: %s", index, err.c_str());
  EXPECT(bits_of(mn) == (int32_t)mn_bits && bits_of(rg) == (int32_t)rg_bits, "float %d: min %g range %g", index, mn, rg);
  std::vector<uint8_t> got(n * code_width(fmt), 0xAB);
  feature_compress(fmt, rows, cols, x.data(), mn, rg, got.data());
  for (size_t i = 0; i < n; i++) {
    long long c = got[i];
    if (fmt == 2) {
      uint16_t c16;
      std::memcpy(&c16, &got[2 * i], 2);
      c = c16;
    }
    if (c != want[i]) {
      EXPECT(c == want[i], "float %d code %zu: %lld, not %lld", index, i, c, want[i]);
      break;
    }
  }
}

static void refusals() {
  const std::vector<uint16_t> pct(4 * 5, 100);
  const std::vector<uint8_t> codes(13 * 5, 7);
  const FeaturePayload good{1, -2.f, 9.f, 13, 5, pct.data(), codes.data()};
  const auto payload = [&](const char *want, int fmt, int D, FeaturePayload p) {
    std::string err;
    const bool ok = feature_payload_check("driver: ", 3, fmt, D, p, &err);
    EXPECT(!ok && err.find(want) != std::string::npos, "wanted \"%s\", got %d \"%s\"", want, (int)ok, err.c_str());
    std::printf("refusal: %s\n", err.c_str());
  };
  const auto with = [&](void (*change)(FeaturePayload &)) {
    FeaturePayload p = good;
    change(p);
    return p;
  };
  payload("driver: item 3 is a payload of format 1, the store holds format 2", 2, 5, good);
  payload("driver: item 3 has 5 columns, feat_dim is 8", 1, 8, good);
  payload("driver: item 3 has 0 rows", 1, 5, with([](FeaturePayload &p) { p.rows = 0; }));
  payload("driver: item 3 has -1 rows", 1, 5, with([](FeaturePayload &p) { p.rows = -1; }));
  payload("driver: item 3: its min or range is not finite", 1, 5, with([](FeaturePayload &p) { p.min_value = std::numeric_limits<float>::quiet_NaN(); }));
  payload("driver: item 3: its min or range is not finite", 1, 5, with([](FeaturePayload &p) { p.range = std::numeric_limits<float>::infinity(); }));
  payload("driver: item 3 comes without codes", 1, 5, with([](FeaturePayload &p) { p.percentiles = nullptr; }));
  const auto matrix = [&](const char *want, int fmt, int rows, int cols, std::vector<float> x) {
    std::string err;
    float mn = -7.f, rg = -7.f;
    const bool ok = feature_compress_check("driver: ", 3, fmt, rows, cols, x.empty() ? nullptr : x.data(), &mn, &rg, &err);
    EXPECT(!ok && err.find(want) != std::string::npos, "wanted \"%s\", got %d \"%s\"", want, (int)ok, err.c_str());
    std::printf("refusal: %s\n", err.c_str());
  };
  matrix("driver: format 1 (CM) from float matrices is not built: Kaldi's percentile selection", 1, 2, 2, {1.f, 2.f, 3.f, 4.f});
  matrix("driver: item 3 has 0 rows", 2, 0, 2, {});
  matrix("driver: item 3: its min or range is not finite", 3, 1, 2, {1.f, std::numeric_limits<float>::infinity()});
  matrix("driver: item 3: its min or range is not finite", 2, 1, 2, {-3e38f, 3e38f});
  const auto lay = [&](const char *want, int fmt, int D, std::vector<int> frames) {
    std::string err;
    std::vector<long long> offsets(frames.size() + 1, -7);
    long long total = -7;
    const bool ok = feature_store_layout("driver: ", fmt, D, (int)frames.size(), frames.data(), offsets.data(), &total, &err);
    EXPECT(!ok && err.find(want) != std::string::npos, "wanted \"%s\", got %d \"%s\"", want, (int)ok, err.c_str());
    for (long long o : offsets) EXPECT(o == -7, "a refused layout wrote offsets");
    EXPECT(total == -7, "a refused layout wrote device_bytes");
    std::printf("refusal: %s\n", err.c_str());
  };
  lay("driver: utterance 1 has 0 frames", 1, 5, {13, 0});
  lay("driver: format 4: a store holds format 1 (CM), 2 (CM2) or 3 (CM3)", 4, 5, {13});
  lay("driver: 2147483648 frames in all: a store holds at most 2^31 - 1", 3, 5, {1 << 30, 1 << 30});
  // ... and what is no refusal: offsets past 2^32 bytes without a byte of memory, a NaN among finite values is skipped by the range
  std::vector<long long> offsets(4);
  long long total = 0;
  std::string err;
  const std::vector<int> big = {500000000, 500000000, 13};
  EXPECT(feature_store_layout("driver: ", 2, 5, 3, big.data(), offsets.data(), &total, &err), "%s", err.c_str());
  EXPECT(offsets[2] == 10000000000LL && offsets[3] == 10000000144LL && total == 10000000144LL + 3 * 32, "%lld %lld %lld", offsets[2], offsets[3], total);
  const std::vector<float> holed = {1.f, std::numeric_limits<float>::quiet_NaN(), 3.f};
  float mn = 0, rg = 0;
  EXPECT(feature_compress_check("driver: ", 0, 3, 1, 3, holed.data(), &mn, &rg, &err) && mn == 1.f && rg == 2.f, "%g %g", mn, rg);
  std::vector<uint8_t> codes3(3, 0xAB);
  feature_compress(3, 1, 3, holed.data(), mn, rg, codes3.data());
  EXPECT(codes3[0] == 0 && codes3[1] == 0 && codes3[2] == 255, "%d %d %d", codes3[0], codes3[1], codes3[2]);
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::string kind;
  int stores = 0, floats = 0;
  while (in >> kind) {
    if (kind == "store") store_case(in, stores++);
    else if (kind == "float") float_case(in, floats++);
    else return 2;
  }
  std::printf("cases: %d stores, %d float matrices\n", stores, floats);
  if (stores == 0 || floats == 0) failures++;
  refusals();
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
