// The dump both text-parse test programs write (tests/text_parse_ref_main.cpp, tests/text_parse_twin_main.cpp) and
// tests/test_text_parse_host.py reads: int64 n_lines, n_rows, nnz, n_slow, first_slow_byte, overflow, then int32
// row_ptr [n_rows + 1], label [n_rows], field [nnz], feat [nnz] and float val [nnz].  n_rows == -1: the text was refused.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

inline bool read_file(const std::string &path, std::vector<char> &out) {
  std::FILE *f = std::fopen(path.c_str(), "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long n = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  out.resize(static_cast<size_t>(n));
  const bool ok = n == 0 || std::fread(out.data(), 1, static_cast<size_t>(n), f) == static_cast<size_t>(n);
  std::fclose(f);
  return ok;
}

inline bool write_dump(const std::string &path, const int64_t head[6], const std::vector<int32_t> &row_ptr, const std::vector<int32_t> &label,
                       const std::vector<int32_t> &field, const std::vector<int32_t> &feat, const std::vector<float> &val) {
  std::FILE *f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  bool ok = std::fwrite(head, sizeof(int64_t), 6, f) == 6;
  auto put = [&](const void *p, size_t n) { ok = ok && (n == 0 || std::fwrite(p, 4, n, f) == n); };
  put(row_ptr.data(), row_ptr.size());
  put(label.data(), label.size());
  put(field.data(), field.size());
  put(feat.data(), feat.size());
  put(val.data(), val.size());
  return std::fclose(f) == 0 && ok;
}
