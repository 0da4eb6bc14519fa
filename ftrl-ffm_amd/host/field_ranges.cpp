#include "field_ranges.h"

#include <charconv>
#include <cstdio>
#include <fstream>
#include <stdexcept>

namespace ftrl {

std::vector<int32_t> uniform_field_ranges(int n_fields, int n_feats) {
  if (n_fields <= 0 || n_feats < n_fields)
    throw std::invalid_argument("--field_ranges uniform needs n_feats >= n_fields (every field owns an id range)");
  std::vector<int32_t> fs(static_cast<size_t>(n_fields) + 1);
  const int per = n_feats / n_fields;
  for (int f = 0; f <= n_fields; f++) fs[f] = f == n_fields ? n_feats : f * per;
  return fs;
}

std::vector<int32_t> read_field_ranges(const std::string &path, int n_fields, int n_feats, bool hashed) {
  std::ifstream in(path);
  if (!in.good()) throw std::invalid_argument(path + ": cannot be opened");
  auto at = [&](size_t line, const std::string &msg) { return std::invalid_argument(path + ":" + std::to_string(line) + ": " + msg); };
  std::vector<int32_t> fs;
  std::string text;
  size_t line = 0;
  const size_t want = static_cast<size_t>(n_fields) + 1;
  while (std::getline(in, text)) {
    line++;
    while (!text.empty() && (text.back() == '\r' || text.back() == ' ' || text.back() == '\t')) text.pop_back();
    if (text.empty()) continue;
    long long v = 0;
    const auto res = std::from_chars(text.data(), text.data() + text.size(), v);
    if (res.ec != std::errc() || res.ptr != text.data() + text.size()) throw at(line, "not an integer: `" + text + "`");
    if (fs.size() == want) throw at(line, "more than n_fields + 1 = " + std::to_string(want) + " values");
    if (fs.empty() && v != 0) throw at(line, "the first value must be 0, got " + text);
    if (v < 0 || v > n_feats) throw at(line, text + " is outside [0, n_feats = " + std::to_string(n_feats) + "]");
    if (!fs.empty() && v < fs.back()) throw at(line, "the values must ascend: " + text + " after " + std::to_string(fs.back()));
    if (!fs.empty() && hashed && v == fs.back())
      throw at(line, "field " + std::to_string(fs.size() - 1) + " has width 0: under --hash_feats every field owns at least one id");
    fs.push_back(static_cast<int32_t>(v));
  }
  if (fs.size() != want)
    throw at(line, std::to_string(fs.size()) + " values, n_fields + 1 = " + std::to_string(want) + " expected");
  if (fs.back() != n_feats) throw at(line, "the last value must be n_feats = " + std::to_string(n_feats) + ", got " + std::to_string(fs.back()));
  return fs;
}

void write_field_ranges(const std::string &path, const std::vector<int32_t> &field_start) {
  std::FILE *f = std::fopen(path.c_str(), "w");
  if (!f) throw std::runtime_error("--field_ranges_out: cannot write " + path);
  bool ok = true;
  for (int32_t v : field_start) ok = ok && std::fprintf(f, "%d\n", v) > 0;
  ok = std::fclose(f) == 0 && ok;
  if (!ok) throw std::runtime_error("--field_ranges_out: writing " + path + " failed");
}

}  // namespace ftrl
