// Stand-alone check of the keep-map file of --rare_ids_out / --rare_ids @FILE (host/rare_ids.cpp; no GPU, no engine
// library): what was written is what is read, and every damaged or mismatching file is refused with a message.
// Built and run by tests/test_rare_ids_host.py from rare_ids.cpp and persist.cpp, once plainly and once under
// -fsanitize=address,undefined.
//   usage: rare_ids_file <scratch directory>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>

#include "../ftrl-ffm_amd/host/persist.h"
#include "../ftrl-ffm_amd/host/rare_ids.h"

static int n_ok = 0, n_fail = 0;
static void check(bool cond, const char *what) {
  std::printf("%s  %s\n", cond ? "ok  " : "FAIL", what);
  (cond ? n_ok : n_fail)++;
}

static std::string slurp(const std::string &path) {
  std::ifstream in(path, std::ios::binary);
  return std::string(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
}
static void spit(const std::string &path, const std::string &bytes) {
  std::ofstream out(path, std::ios::binary | std::ios::trunc);
  out.write(bytes.data(), static_cast<std::streamsize>(bytes.size()));
}
// The message read_rare_ids refuses the file with; "" when it reads it.
static std::string refusal(const std::string &path, int n_fields, int bits) {
  try {
    ftrl::read_rare_ids(path, n_fields, bits);
  } catch (const std::invalid_argument &e) {
    return e.what();
  }
  return "";
}
static bool has(const std::string &msg, const std::string &path, const char *part) {
  return msg.find(path) != std::string::npos && msg.find(part) != std::string::npos;
}

static ftrl::RareIds make(int bits, int n_fields, int min_count) {
  ftrl::RareIds m;
  m.bits = bits;
  m.n_fields = n_fields;
  m.min_count = min_count;
  m.rows = 123456789012ull;
  m.words.resize((static_cast<size_t>(1) << bits) / 64);
  uint64_t x = 88172645463325252ull;  // xorshift64
  for (auto &w : m.words) {
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
    w = x;
  }
  m.words[0] = 0x8000000000000001ull;  // (both ends of a word)
  m.words.back() = 0;
  return m;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  if (!ftrl::zstd_available()) {
    std::printf("FAIL  libzstd is not available\n");
    return 1;
  }
  const std::string dir = argv[1];
  const std::string a = dir + "/a.rare", b = dir + "/b.rare", bad = dir + "/bad.rare";

  const ftrl::RareIds small = make(8, 5, 3);
  ftrl::write_rare_ids(a, small);
  ftrl::RareIds got = ftrl::read_rare_ids(a, 5, 0);
  uint64_t bits_set = 0;
  for (uint64_t w : small.words) bits_set += static_cast<uint64_t>(__builtin_popcountll(w));
  check(got.words == small.words && got.bits == 8 && got.min_count == 3 && got.n_fields == 5 && got.rows == small.rows &&
            got.kept_slots == bits_set,
        "round trip: 2^8 slots, 5 fields");
  check(ftrl::read_rare_ids(a, 5, 8).words == small.words, "the file's own --rare_bits is accepted");
  const ftrl::RareIds large = make(16, 0, 65535);
  ftrl::write_rare_ids(b, large);
  got = ftrl::read_rare_ids(b, 0, 0);
  check(got.words == large.words && got.bits == 16 && got.n_fields == 0 && got.min_count == 65535, "round trip: 2^16 slots, LR / FM");
  check(slurp(b).size() < 48 + 8 * large.words.size() + 64 && slurp(a).size() > 48, "a 48-byte header and one frame");

  std::vector<uint64_t> flipped = small.words;
  flipped[2] ^= 1ull << 40;
  check(ftrl::rare_ids_checksum(flipped) != ftrl::rare_ids_checksum(small.words) &&
            ftrl::rare_ids_checksum(std::vector<uint64_t>()) == 14695981039346656037ull,
        "the checksum sees one bit");
  check(ftrl::default_rare_bits(10000) == 16 && ftrl::default_rare_bits(16384) == 16 && ftrl::default_rare_bits(16385) == 17 &&
            ftrl::default_rare_bits(1 << 20) == 22 && ftrl::default_rare_bits(1 << 28) == 30 && ftrl::default_rare_bits(2147483647) == 30 &&
            ftrl::default_rare_bits(1) == 16,
        "--rare_bits' default: 2^B >= 4 * n_feats inside [16, 30]");

  check(has(refusal(dir + "/none.rare", 5, 0), "none.rare", "cannot be opened"), "refused: no such file");
  const std::string bytes = slurp(a);
  std::string damaged = bytes;
  damaged[3] = 'X';
  spit(bad, damaged);
  check(has(refusal(bad, 5, 0), bad, "wrong magic"), "refused: wrong magic");
  spit(bad, bytes.substr(0, 30));
  check(has(refusal(bad, 5, 0), bad, "header is truncated"), "refused: truncated header");
  spit(bad, bytes.substr(0, bytes.size() - 7));
  check(has(refusal(bad, 5, 0), bad, "truncated"), "refused: truncated frame");
  damaged = bytes;
  damaged[40] = static_cast<char>(damaged[40] ^ 0x10);  // (a byte of the header's checksum)
  spit(bad, damaged);
  check(has(refusal(bad, 5, 0), bad, "checksum"), "refused: wrong checksum");
  check(has(refusal(a, 6, 0), a, "5 fields") && has(refusal(a, 0, 0), a, "5 fields") && has(refusal(b, 5, 0), b, "without fields"),
        "refused: another n_fields");
  damaged = bytes;
  damaged[12] = 9;  // (the header's bits: 2^9 slots, the frame still holds 2^8 / 64 words)
  spit(bad, damaged);
  check(has(refusal(bad, 5, 0), bad, "the frame holds 4 words") && has(refusal(bad, 5, 0), bad, "imply 8"), "refused: bits against the frame's words");
  check(has(refusal(a, 5, 12), a, "--rare_bits asks for 2^12"), "refused: other --rare_bits than the file's");
  damaged = bytes;
  damaged[8] = 2;  // (the version)
  spit(bad, damaged);
  check(has(refusal(bad, 5, 0), bad, "version 2"), "refused: another version");
  bool threw = false;
  try {
    ftrl::RareIds m = small;
    m.words.pop_back();
    ftrl::write_rare_ids(bad, m);
  } catch (const std::invalid_argument &) {
    threw = true;
  }
  check(threw, "write refuses words that are not 2^bits / 64");
  std::printf("%d ok, %d failed\n", n_ok, n_fail);
  return n_fail == 0 ? 0 : 1;
}
