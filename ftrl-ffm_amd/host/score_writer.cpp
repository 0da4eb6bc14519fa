#include "score_writer.h"

#include <charconv>
#include <cmath>
#include <cstring>

namespace ftrl {

size_t format_score(float v, char *buf) {
  if (std::isnan(v)) { std::memcpy(buf, "nan", 3); return 3; }
  if (std::isinf(v)) {
    const bool neg = std::signbit(v);
    std::memcpy(buf, neg ? "-inf" : "inf", neg ? 4 : 3);
    return neg ? 4 : 3;
  }
#if defined(__cpp_lib_to_chars) && __cpp_lib_to_chars >= 201611L
  // (the overload without a format: the shortest text that round-trips)
  const std::to_chars_result r = std::to_chars(buf, buf + kScoreTextMax, v);
  return static_cast<size_t>(r.ptr - buf);
#else
  // (a toolchain without floating-point to_chars: nine significant digits always round-trip a float)
  return static_cast<size_t>(std::snprintf(buf, kScoreTextMax, "%.9g", static_cast<double>(v)));
#endif
}

void append_scores(const float *v, size_t n, std::string &out) {
  char buf[kScoreTextMax];
  out.reserve(out.size() + n * 12);
  for (size_t i = 0; i < n; i++) {
    const size_t len = format_score(v[i], buf);
    buf[len] = '\n';
    out.append(buf, len + 1);
  }
}

bool write_scores(std::FILE *f, const float *v, size_t n, std::string &scratch) {
  scratch.clear();
  append_scores(v, n, scratch);
  return std::fwrite(scratch.data(), 1, scratch.size(), f) == scratch.size();
}

}  // namespace ftrl
