// Stand-alone program (no GPU, no engine library): the CLI's REAL parser, parse_csr_range of host/csr_reader.cpp,
// over whole files, dumped as tests/text_parse_dump.h says.  Built from host/csr_reader.cpp and host/csr_stream.cpp
// and run by tests/test_text_parse_host.py, which holds the host twin of the device grammar against it.
//   usage: text_parse_ref <has_field 0|1> <text file> <dump file> [<text file> <dump file> ...]
#include <cstdlib>
#include <stdexcept>

#include "../ftrl-ffm_amd/host/csr_reader.h"
#include "text_parse_dump.h"

int main(int argc, char **argv) {
  if (argc < 4 || (argc - 2) % 2 != 0) return 2;
  const bool has_field = std::atoi(argv[1]) != 0;
  for (int i = 2; i + 1 < argc; i += 2) {
    std::vector<char> text;
    if (!read_file(argv[i], text)) return 2;
    ftrl::CsrPart part;
    int64_t head[6] = {-1, 0, 0, 0, -1, 0};
    std::vector<int32_t> row_ptr;
    try {
      ftrl::parse_csr_range(text.data(), text.data() + text.size(), has_field, part);
      row_ptr.push_back(0);
      for (int32_t n : part.nnz) row_ptr.push_back(row_ptr.back() + n);
      head[1] = static_cast<int64_t>(part.nnz.size());
      head[2] = static_cast<int64_t>(part.feat.size());
    } catch (const std::out_of_range &) {  // (`wrong input: ...` is on stdout)
      part.clear();
      head[1] = -1;
    }
    if (!write_dump(argv[i + 1], head, row_ptr, part.label, part.field, part.feat, part.val)) return 2;
  }
  return 0;
}
