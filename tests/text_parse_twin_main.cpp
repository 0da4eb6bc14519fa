// Stand-alone program (no GPU, no engine library): the host twin of the device text grammar,
// ftrl_text::parse_block_host of csrc/text_parse.h, over whole files, dumped as tests/text_parse_dump.h says.  Built
// with a plain C++ compiler and run by tests/test_text_parse_host.py, once under -fsanitize=address,undefined; the
// arrays are allocated at exactly the capacities given, so a store past them is a finding.
//   usage: text_parse_twin <has_field 0|1> <max_rows | -1> <max_nnz | -1> <text file> <dump file> [<text file> <dump file> ...]
#include <cstdlib>

#include "../ftrl-ffm_amd/csrc/text_parse.h"
#include "text_parse_dump.h"

int main(int argc, char **argv) {
  if (argc < 6 || (argc - 4) % 2 != 0) return 2;
  const bool has_field = std::atoi(argv[1]) != 0;
  const long cap_rows = std::atol(argv[2]), cap_nnz = std::atol(argv[3]);
  for (int i = 4; i + 1 < argc; i += 2) {
    std::vector<char> text;
    if (!read_file(argv[i], text)) return 2;
    const int32_t n = static_cast<int32_t>(text.size());
    const int32_t max_rows = cap_rows < 0 ? n / 2 + 1 : static_cast<int32_t>(cap_rows);
    const int32_t max_nnz = cap_nnz < 0 ? n / 4 + 1 : static_cast<int32_t>(cap_nnz);
    std::vector<int32_t> row_ptr(static_cast<size_t>(max_rows) + 1), label(static_cast<size_t>(max_rows)), field(static_cast<size_t>(max_nnz)),
        feat(static_cast<size_t>(max_nnz));
    std::vector<float> val(static_cast<size_t>(max_nnz));
    const ftrl_text::Totals t =
        ftrl_text::parse_block_host(has_field, text.data(), n, max_rows, max_nnz, row_ptr.data(), field.data(), feat.data(), val.data(), label.data());
    const int64_t head[6] = {t.n_lines, t.n_rows, t.nnz, t.n_slow, t.first_slow_byte, t.overflow};
    const bool valid = t.n_slow == 0 && !t.overflow;
    const size_t r = valid ? static_cast<size_t>(t.n_rows) : 0, e = valid ? static_cast<size_t>(t.nnz) : 0;
    row_ptr.resize(valid ? r + 1 : 0);
    label.resize(r);
    field.resize(e);
    feat.resize(e);
    val.resize(e);
    if (!write_dump(argv[i + 1], head, row_ptr, label, field, feat, val)) return 2;
  }
  return 0;
}
