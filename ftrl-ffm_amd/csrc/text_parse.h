// text_parse.h -- the grammar of libffm / libsvm text that is parsed WITHOUT the host parser, IDENTICAL BITS on the
// device (kernels_text.h) and on the host (ffm_engine_textparse_host, and whoever includes this header with a plain
// C++ compiler).  The contract is stated in include/ffm_engine.h, "Text blocks".
//
// It restates what parse_range (host/csr_reader.cpp) does for lines that stay on its fast path, rule by rule:
//
// Text blocks
//   lines    a line ends at '\n' or at the end of the text (csr_reader.cpp:105-106: memchr, else `end`), so a last
//            line without a newline is a line; one trailing '\r' is stripped (:109); the only blank is ' ' (:110,
//            :113, :119); a line with nothing but blanks yields no row (:111).
//   label    the first token (:112-114).  Here: optional '+' or '-', then 1 to 9 digits, and nothing else in the
//            token -- a subset of what to_int takes (:33-39: an optional '+', then from_chars, which takes a '-'
//            and stops at the first non-digit).  The row's label is 1 if the value is > 0, else 0 (:114).
//   entries  field:feat:value when has_field, else feat:value with field written as 0 (:67-73); ids are 1 to 9
//            digits (fast_uint, :56-63); the value is [-]digits[.digits] (:74-95), "1." and ".5" included (only
//            n_any == 0 is refused, :96), of at most 7 significant digits (:83, :93) and at most 10 fraction digits
//            (:93); the token ends at a blank or the line's end (:96); the value is float(digits) / 10^n_frac,
//            negated if signed (:97-98) -- one correctly rounded division of two exact floats; an entry whose value
//            compares equal to 0.0f is dropped, -0 too (:125).
//   slow     any other line.  It is not parsed and nothing is guessed: it counts in n_slow, gives no row and no
//            entry, and the caller hands its text to the host parser.  That is everything fast_token returns
//            false for (an exponent, nan, inf, a tab, a '+' on a value, a missing part, a 10-digit id), a label
//            outside the grammar above, and a line of more than kMaxLine bytes before its '\n'.
//
// Positions are 32-bit: a text is shorter than 2^31 bytes (ffm_engine_textparse_create refuses more).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FTRL_TEXT_HD __host__ __device__ __forceinline__
#else
#define FTRL_TEXT_HD inline
#endif

namespace ftrl_text {

constexpr int32_t kMaxLine = 65536;  // FFM_TEXT_MAX_LINE

FTRL_TEXT_HD bool is_digit(char c) { return static_cast<unsigned>(c - '0') <= 9u; }

// fast_uint: 1 to 9 digits at t[c ..), c moved behind them.
FTRL_TEXT_HD bool parse_uint(const char *t, int32_t &c, int32_t stop, int32_t &v) {
  const int32_t b = c;
  uint32_t x = 0;
  while (c < stop && is_digit(t[c])) {
    if (c - b < 9) x = x * 10u + static_cast<uint32_t>(t[c] - '0');  // (a tenth digit refuses the token below)
    c++;
  }
  if (c == b || c - b > 9) return false;
  v = static_cast<int32_t>(x);
  return true;
}

// The label token at t[q ..): false = outside the grammar (the line is slow).
FTRL_TEXT_HD bool parse_label(const char *t, int32_t q, int32_t stop, int32_t &label) {
  int32_t c = q;
  bool neg = false;
  if (c < stop && (t[c] == '+' || t[c] == '-')) {
    neg = t[c] == '-';
    c++;
  }
  int32_t v = 0;
  if (!parse_uint(t, c, stop, v)) return false;
  if (c < stop && t[c] != ' ') return false;
  label = (!neg && v > 0) ? 1 : 0;
  return true;
}

// fast_token: one entry token at t[q ..), q on a non-blank.  false = outside the grammar (the line is slow).
FTRL_TEXT_HD bool parse_entry(const char *t, int32_t q, int32_t stop, bool has_field, int32_t &fld, int32_t &ft, float &v) {
  int32_t c = q;
  fld = 0;
  if (has_field) {
    if (!parse_uint(t, c, stop, fld) || c >= stop || t[c] != ':') return false;
    c++;
  }
  if (!parse_uint(t, c, stop, ft) || c >= stop || t[c] != ':') return false;
  c++;
  bool neg = false;
  if (c < stop && t[c] == '-') {
    neg = true;
    c++;
  }
  uint32_t digits = 0;     // the significand as an integer, < 10^7 < 2^24: an exact float
  uint64_t pow10 = 1;      // 10^n_frac <= 10^10 = 2^10 * 5^10, 5^10 < 2^24: an exact float
  int32_t n_sig = 0, n_frac = 0, n_any = 0;
  while (c < stop && is_digit(t[c])) {
    digits = digits * 10u + static_cast<uint32_t>(t[c] - '0');
    n_sig += (n_sig > 0 || t[c] != '0') ? 1 : 0;
    n_any++;
    c++;
    if (n_sig > 7) return false;
  }
  if (c < stop && t[c] == '.') {
    c++;
    while (c < stop && is_digit(t[c])) {
      digits = digits * 10u + static_cast<uint32_t>(t[c] - '0');
      n_sig += (n_sig > 0 || t[c] != '0') ? 1 : 0;
      n_any++;
      n_frac++;
      pow10 *= 10u;
      c++;
      if (n_sig > 7 || n_frac > 10) return false;
    }
  }
  if (n_any == 0 || (c < stop && t[c] != ' ')) return false;
  const float mag = n_frac ? static_cast<float>(digits) / static_cast<float>(pow10) : static_cast<float>(digits);
  v = neg ? -mag : mag;
  return true;
}

// What one text came to (ffm_text_block's counts).
struct Totals {
  int64_t n_lines = 0, n_rows = 0, nnz = 0, n_slow = 0, first_slow_byte = -1;
  int32_t overflow = 0;
};

// The whole grammar on the host, line by line: the counts always, the arrays (row_ptr [max_rows + 1], label
// [max_rows], field / feat / val [max_nnz]) valid when n_slow == 0 and overflow == 0.  A slow line gives no row and
// no entry.  Nothing is stored past the capacities.
inline Totals parse_block_host(bool has_field, const char *t, int32_t n_bytes, int32_t max_rows, int32_t max_nnz, int32_t *row_ptr,
                               int32_t *field, int32_t *feat, float *val, int32_t *label) {
  Totals out;
  int32_t p = 0;
  while (p < n_bytes) {
    int32_t le = p;
    while (le < n_bytes && t[le] != '\n') le++;
    const int32_t lb = p;
    p = le + 1;
    out.n_lines++;
    bool slow = le - lb > kMaxLine;
    int64_t kept = 0;
    int32_t lab = 0;
    bool is_row = false;
    if (!slow) {
      int32_t stop = le, q = lb;
      if (stop > lb && t[stop - 1] == '\r') stop--;
      while (q < stop && t[q] == ' ') q++;
      if (q < stop) {
        is_row = true;
        slow = !parse_label(t, q, stop, lab);
        while (q < stop && t[q] != ' ') q++;
        while (!slow) {
          while (q < stop && t[q] == ' ') q++;
          if (q >= stop) break;
          int32_t fld, ft;
          float v;
          if (!parse_entry(t, q, stop, has_field, fld, ft, v)) {
            slow = true;
            break;
          }
          if (v != 0.0f) {
            const int64_t at = out.nnz + kept;
            if (at < max_nnz && out.n_rows < max_rows) {
              field[at] = fld;
              feat[at] = ft;
              val[at] = v;
            }
            kept++;
          }
          while (q < stop && t[q] != ' ') q++;
        }
      }
    }
    if (slow) {
      if (out.n_slow++ == 0) out.first_slow_byte = lb;
      continue;
    }
    if (!is_row) continue;
    if (out.n_rows < max_rows) {
      row_ptr[out.n_rows] = static_cast<int32_t>(out.nnz < max_nnz ? out.nnz : max_nnz);
      label[out.n_rows] = lab;
    }
    out.n_rows++;
    out.nnz += kept;
  }
  out.overflow = (out.n_rows > max_rows || out.nnz > max_nnz) ? 1 : 0;
  if (!out.overflow) row_ptr[out.n_rows] = static_cast<int32_t>(out.nnz);
  return out;
}

}  // namespace ftrl_text
