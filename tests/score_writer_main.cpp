// score_writer_main.cpp -- stand-alone check of host/score_writer.{h,cpp} (floats -> one line of text
// each): built by tests/test_score_writer.py with g++ alone, plainly and with
// -fsanitize=address,undefined, and run directly.  Every line must parse back (strtof) to the bits
// it was written from; a NaN only to a NaN.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../ftrl-ffm_amd/host/score_writer.h"

static int n_checks = 0, n_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    n_checks++;                                                            \
    if (!(cond)) {                                                         \
      n_failed++;                                                          \
      if (n_failed <= 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                      \
  } while (0)

static uint32_t bits_of(float v) { uint32_t b; std::memcpy(&b, &v, 4); return b; }
static float from_bits(uint32_t b) { float v; std::memcpy(&v, &b, 4); return v; }

int main() {
  std::vector<float> v;
  const uint32_t special[] = {
      0x00000000u, 0x80000000u,                            // +0, -0
      0x00000001u, 0x80000001u, 0x007fffffu, 0x807fffffu,  // the smallest and the largest subnormals
      0x00012345u, 0x00400000u,                            // subnormals in between
      0x00800000u, 0x80800000u,                            // FLT_MIN
      0x7f7fffffu, 0xff7fffffu,                            // FLT_MAX
      0x7f800000u, 0xff800000u,                            // inf
      0x7fc00000u, 0xffc00000u, 0x7f800001u, 0x7fffffffu,  // NaNs: quiet, negative, signalling, full payload
      0x3f800000u, 0x3f000000u, 0x3dcccccdu, 0x3f7fffffu, 0x33800000u};  // 1, 0.5, 0.1f, 1 - ulp, 2^-24
  for (uint32_t b : special) v.push_back(from_bits(b));
  std::mt19937 rng(12345);
  for (int i = 0; i < 100000; i++) v.push_back(from_bits(static_cast<uint32_t>(rng())));
  // sigmoid-like values too: what the CLI writes
  std::uniform_real_distribution<float> u01(0.0f, 1.0f);
  for (int i = 0; i < 20000; i++) v.push_back(u01(rng));

  CHECK(v[6] == from_bits(0x00012345u) && FLT_MAX == from_bits(0x7f7fffffu));

  // one value at a time: length within the bound, nothing written behind it
  size_t longest = 0;
  for (float x : v) {
    char buf[ftrl::kScoreTextMax + 8];
    std::memset(buf, '#', sizeof buf);
    const size_t len = ftrl::format_score(x, buf);
    CHECK(len > 0 && len < ftrl::kScoreTextMax);
    bool clean = true;
    for (size_t i = ftrl::kScoreTextMax; i < sizeof buf; i++) clean = clean && buf[i] == '#';
    CHECK(clean);
    if (len > longest) longest = len;
  }
  CHECK(longest <= 16);

  // the span at once: one line per value, in order, each parsing back to the same bits
  std::string text = "head\n";
  ftrl::append_scores(v.data(), v.size(), text);
  CHECK(text.compare(0, 5, "head\n") == 0);
  size_t pos = 5, line = 0;
  while (pos < text.size()) {
    const size_t end = text.find('\n', pos);
    CHECK(end != std::string::npos);
    if (end == std::string::npos || line >= v.size()) break;
    const std::string s = text.substr(pos, end - pos);
    char *stop = nullptr;
    const float back = std::strtof(s.c_str(), &stop);
    CHECK(stop == s.c_str() + s.size());  // the whole line is the number
    const float want = v[line];
    if (std::isnan(want)) {
      CHECK(std::isnan(back));
      CHECK(s == "nan");
    } else {
      CHECK(bits_of(back) == bits_of(want));
      if (std::isinf(want)) CHECK(s == (want > 0 ? "inf" : "-inf"));
    }
    pos = end + 1;
    line++;
  }
  CHECK(line == v.size());

  // an empty span appends nothing; the FILE writer writes the same bytes
  std::string none = "x";
  ftrl::append_scores(nullptr, 0, none);
  CHECK(none == "x");
  std::FILE *f = std::tmpfile();
  CHECK(f != nullptr);
  if (f) {
    std::string scratch = "stale";
    CHECK(ftrl::write_scores(f, v.data(), v.size(), scratch));
    CHECK(ftrl::write_scores(f, v.data(), 0, scratch));
    std::fflush(f);
    const long size = std::ftell(f);
    CHECK(size == static_cast<long>(text.size() - 5));
    std::rewind(f);
    std::string file(static_cast<size_t>(size > 0 ? size : 0), '\0');
    CHECK(std::fread(&file[0], 1, file.size(), f) == file.size());
    CHECK(file == text.substr(5));
    std::fclose(f);
  }
  // a few spellings the shortest form must give
  auto one = [](float x) { char b[ftrl::kScoreTextMax]; return std::string(b, ftrl::format_score(x, b)); };
  CHECK(one(0.5f) == "0.5" && one(1.0f) == "1" && one(0.1f) == "0.1" && one(-0.0f) == "-0");

  std::printf("%d checks, %d failed\n", n_checks, n_failed);
  return n_failed ? 1 : 0;
}
