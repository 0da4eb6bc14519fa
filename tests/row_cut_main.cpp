// Stand-alone program (no GPU, no engine library): the block planner of host/row_cut.h -- which sees nothing of a
// chunk but its row_ptr -- against CsrStream::next (host/csr_stream.cpp), the cut rule it restates.  The text is cut
// into chunks of whole lines the way host/text_stream.cpp cuts a file into slots, every chunk is parsed by the host
// twin of the device grammar (csrc/text_parse.h) for its row_ptr, and the planner's blocks must be CsrStream's: the
// same rows and the same entries per block.  Built and run by tests/test_row_cut_host.py, once plainly and once under
// -fsanitize=address,undefined.
//   usage: row_cut <has_field 0|1> <text file> <chunk_bytes> <want> <max_nnz | -1> [<chunk_bytes> <want> <max_nnz> ...]
// Per case one line: `case <chunk_bytes> <want> <max_nnz>: B blocks, C chunks, inside I, two T, three+ M, feeds F`
// (blocks inside one chunk / spanning two / spanning three or more; the most blocks one chunk feeds), or
// `case ...: length_error <text>` where both refuse a row over the budget with the same text.  Exit status 1 and a
// `MISMATCH` line where they differ.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../ftrl-ffm_amd/csrc/text_parse.h"
#include "../ftrl-ffm_amd/host/csr_stream.h"
#include "../ftrl-ffm_amd/host/row_cut.h"
#include "text_parse_dump.h"

struct Block {
  size_t rows = 0, nnz = 0;
};

int main(int argc, char **argv) {
  if (argc < 6 || (argc - 3) % 3 != 0) return 2;
  const bool has_field = std::atoi(argv[1]) != 0;
  const std::string path = argv[2];
  std::vector<char> text;
  if (!read_file(path, text)) return 2;
  int bad = 0;
  for (int a = 3; a + 2 < argc; a += 3) {
    const size_t chunk_bytes = static_cast<size_t>(std::atol(argv[a])), want = static_cast<size_t>(std::atol(argv[a + 1]));
    const long budget = std::atol(argv[a + 2]);
    const size_t max_nnz = budget < 0 ? static_cast<size_t>(-1) : static_cast<size_t>(budget);
    // the chunks: whole lines, at most chunk_bytes (a longer single line alone), and each one's row_ptr
    std::vector<std::vector<int32_t>> row_ptrs;
    std::vector<ftrl::RowCutChunk> chunks;
    for (size_t at = 0; at < text.size();) {
      size_t end = std::min(text.size(), at + chunk_bytes);
      if (end < text.size()) {
        size_t cut = end;
        while (cut > at && text[cut - 1] != '\n') cut--;
        if (cut == at) {
          const void *nl = std::memchr(text.data() + end, '\n', text.size() - end);
          cut = nl ? static_cast<size_t>(static_cast<const char *>(nl) - text.data()) + 1 : text.size();
        }
        end = cut;
      }
      const int32_t n = static_cast<int32_t>(end - at), max_rows = n / 2 + 1, cap_nnz = n / 4 + 2;
      std::vector<int32_t> row_ptr(static_cast<size_t>(max_rows) + 1), label(static_cast<size_t>(max_rows)), field(static_cast<size_t>(cap_nnz)),
          feat(static_cast<size_t>(cap_nnz));
      std::vector<float> val(static_cast<size_t>(cap_nnz));
      const ftrl_text::Totals t = ftrl_text::parse_block_host(has_field, text.data() + at, n, max_rows, cap_nnz, row_ptr.data(), field.data(),
                                                              feat.data(), val.data(), label.data());
      if (t.n_slow != 0 || t.overflow) {
        std::printf("a chunk at byte %zu is outside the grammar\n", at);
        return 2;
      }
      row_ptr.resize(static_cast<size_t>(t.n_rows) + 1);
      row_ptrs.push_back(std::move(row_ptr));
      at = end;
    }
    for (const auto &rp : row_ptrs) {
      ftrl::RowCutChunk c;
      c.row_ptr = rp.data();
      c.n_rows = rp.size() - 1;
      chunks.push_back(c);
    }
    // the planner's blocks, and what they span
    std::vector<Block> mine;
    std::string my_error;
    size_t inside = 0, two = 0, more = 0, feeds = 0, asked = 0;
    std::map<size_t, size_t> fed;
    try {
      ftrl::RowCutCursor cur;
      for (;;) {
        size_t first = static_cast<size_t>(-1), last = 0, rows_seen = 0, nnz = 0;
        const size_t got = ftrl::plan_block(
            want, max_nnz, true, cur,
            [&](size_t ordinal) -> const ftrl::RowCutChunk * {
              if (ordinal < asked) {  // (never back behind a chunk it has left)
                std::printf("MISMATCH the planner asked for chunk %zu after chunk %zu\n", ordinal, asked);
                bad = 1;
              }
              asked = ordinal;
              return ordinal < chunks.size() ? &chunks[ordinal] : nullptr;
            },
            [&](const ftrl::RowSegment &s) {
              if (s.r1 <= s.r0 || s.r1 > chunks[s.chunk].n_rows || s.nnz != static_cast<size_t>(chunks[s.chunk].row_ptr[s.r1] - chunks[s.chunk].row_ptr[s.r0])) {
                std::printf("MISMATCH a segment outside its chunk\n");
                bad = 1;
              }
              first = std::min(first, s.chunk);
              last = std::max(last, s.chunk);
              rows_seen += s.r1 - s.r0;
              fed[s.chunk]++;
            },
            &nnz);
        if (got == 0) break;
        if (rows_seen != got) {
          std::printf("MISMATCH the segments hold %zu rows, the block %zu\n", rows_seen, got);
          bad = 1;
        }
        const size_t span = last - first + 1;
        (span == 1 ? inside : span == 2 ? two : more)++;
        Block b;
        b.rows = got;
        b.nnz = nnz;
        mine.push_back(b);
      }
    } catch (const std::length_error &e) {
      my_error = e.what();
    }
    for (const auto &kv : fed) feeds = std::max(feeds, kv.second);
    // CsrStream's
    std::vector<Block> ref;
    std::string ref_error;
    try {
      ftrl::CsrStream stream(path, has_field ? "libffm" : "libsvm", 2);
      CsrBlock blk;
      for (;;) {
        const size_t got = stream.next(want, blk, max_nnz, true);
        if (got == 0) break;
        Block b;
        b.rows = got;
        b.nnz = blk.feat.size();
        ref.push_back(b);
      }
    } catch (const std::length_error &e) {
      ref_error = e.what();
    }
    std::printf("case %zu %zu %ld: ", chunk_bytes, want, budget);
    if (my_error != ref_error) {
      std::printf("MISMATCH errors `%s` and `%s`\n", my_error.c_str(), ref_error.c_str());
      bad = 1;
      continue;
    }
    // (a refusal ends both at the same block: what came before it is compared too)
    bool same = mine.size() == ref.size();
    for (size_t i = 0; same && i < mine.size(); i++) same = mine[i].rows == ref[i].rows && mine[i].nnz == ref[i].nnz;
    if (!same) {
      std::printf("MISMATCH %zu blocks against %zu\n", mine.size(), ref.size());
      bad = 1;
      continue;
    }
    if (!my_error.empty()) std::printf("length_error %s\n", my_error.c_str());
    else std::printf("%zu blocks, %zu chunks, inside %zu, two %zu, three+ %zu, feeds %zu\n", mine.size(), chunks.size(), inside, two, more, feeds);
  }
  return bad;
}
