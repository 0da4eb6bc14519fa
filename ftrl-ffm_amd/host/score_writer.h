// score_writer.h -- predictions as text, one per line (the CLI's --predict_out).  Knows nothing of
// the engine: it formats a span of floats.
//
// A finite value is written as the shortest decimal that parses back (strtof) to the same float;
// the others as "nan", "inf", "-inf" (a NaN's sign and payload are not kept).
#pragma once
#include <cstddef>
#include <cstdio>
#include <string>

namespace ftrl {

constexpr size_t kScoreTextMax = 24;  // the longest line ("-3.4028235e+38\n" is 15), with room to spare

// One value without a line end into buf[kScoreTextMax]; returns its length (no terminating NUL).
size_t format_score(float v, char *buf);
// n values, one line each, appended to `out`.
void append_scores(const float *v, size_t n, std::string &out);
// n values, one line each, to `f`; false when the write failed.
bool write_scores(std::FILE *f, const float *v, size_t n, std::string &scratch);

}  // namespace ftrl
