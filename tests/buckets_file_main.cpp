// Stand-alone check of the bucket table file of --buckets_out / --buckets @FILE (host/value_buckets.cpp; no GPU, no
// engine library): what was written is what is read, and every damaged or mismatching file is refused with a message
// that names the path.  Built and run by tests/test_value_buckets_host.py from value_buckets.cpp, once plainly and
// once under -fsanitize=address,undefined.
//   usage: buckets_file <scratch directory>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>

#include "../ftrl-ffm_amd/host/value_buckets.h"

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
// The message read_value_buckets refuses the file with; "" when it reads it.
static std::string refusal(const std::string &path, int n_fields) {
  try {
    ftrl::read_value_buckets(path, n_fields);
  } catch (const std::invalid_argument &e) {
    return e.what();
  }
  return "";
}
static bool has(const std::string &msg, const std::string &path, const char *part) {
  return msg.find(path) != std::string::npos && msg.find(part) != std::string::npos;
}
static void set(ftrl::ValueBuckets &t, int f, const std::vector<int> &e) {
  t.n_edges[static_cast<size_t>(f)] = static_cast<int32_t>(e.size());
  for (size_t i = 0; i < e.size(); i++) t.edges[static_cast<size_t>(f) * ftrl::kBucketMaxEdges + i] = static_cast<uint16_t>(e[i]);
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  const std::string dir = argv[1];
  const std::string a = dir + "/a.buckets", bad = dir + "/bad.buckets";

  ftrl::ValueBuckets t(8);
  set(t, 1, {0, 32768, 65535});
  set(t, 3, {});
  std::vector<int> all;
  for (int i = 0; i < 255; i++) all.push_back(100 + 2 * i);
  set(t, 7, all);
  ftrl::write_value_buckets(a, t);
  const ftrl::ValueBuckets got = ftrl::read_value_buckets(a, 8);
  bool same = got.n_fields == 8 && got.n_edges == t.n_edges;
  for (int f : {1, 3, 7})
    for (int i = 0; i < t.n_edges[static_cast<size_t>(f)]; i++)
      same = same && got.edges[static_cast<size_t>(f) * 255 + static_cast<size_t>(i)] == t.edges[static_cast<size_t>(f) * 255 + static_cast<size_t>(i)];
  check(same && got.n_edges[0] == -1 && got.n_edges[3] == 0 && got.n_edges[7] == 255, "round trip: 3, 0 and 255 edges, the other fields not bucketed");
  const std::string text = slurp(a);
  check(text.rfind("FFMBUCKETS 1 8\n1 3 0 32768 65535\n3 0\n7 255 100 102 ", 0) == 0, "the file is text: a header line, then `f k e1 .. ek`");
  spit(bad, text + "\n  \n");
  check(refusal(bad, 8).empty(), "blank lines at the end are fine");

  check(has(refusal(dir + "/none.buckets", 8), "none.buckets", "cannot be opened"), "refused: no such file");
  spit(bad, "");
  check(has(refusal(bad, 8), bad, "empty file"), "refused: an empty file");
  spit(bad, "FFMBUCKETZ 1 8\n1 1 5\n");
  check(has(refusal(bad, 8), bad, "wrong magic"), "refused: wrong magic");
  spit(bad, "FFMBUCKETS 2 8\n1 1 5\n");
  check(has(refusal(bad, 8), bad, "version 2"), "refused: another version");
  spit(bad, "FFMBUCKETS 1\n1 1 5\n");
  check(has(refusal(bad, 8), bad, "header is damaged"), "refused: a header without n_fields");
  check(has(refusal(a, 9), a, "8 fields") && has(refusal(a, 9), a, "this model has 9"), "refused: another n_fields");
  spit(bad, "FFMBUCKETS 1 8\n8 1 5\n");
  check(has(refusal(bad, 8), bad, "field 8 is outside [0, 8)"), "refused: a field outside [0, n_fields)");
  spit(bad, "FFMBUCKETS 1 8\n-1 1 5\n");
  check(has(refusal(bad, 8), bad, "outside [0, 8)"), "refused: a negative field");
  spit(bad, "FFMBUCKETS 1 8\n2 1 5\n2 1 6\n");
  check(has(refusal(bad, 8), bad, "named twice"), "refused: a field named twice");
  spit(bad, "FFMBUCKETS 1 8\n2 3 5 9 9\n");
  check(has(refusal(bad, 8), bad, "strictly ascending") && has(refusal(bad, 8), bad, "line 2"), "refused: edges that repeat");
  spit(bad, "FFMBUCKETS 1 8\n2 3 5 9 7\n");
  check(has(refusal(bad, 8), bad, "strictly ascending"), "refused: edges that descend");
  spit(bad, "FFMBUCKETS 1 8\n2 3 5 9\n");
  check(has(refusal(bad, 8), bad, "fewer than its 3 edges"), "refused: a truncated line");
  spit(bad, "FFMBUCKETS 1 8\n2 2 5 9 11\n");
  check(has(refusal(bad, 8), bad, "more than its 2 edges"), "refused: more edges than the count");
  spit(bad, "FFMBUCKETS 1 8\n2 256 5\n");
  check(has(refusal(bad, 8), bad, "0 .. 255 edges"), "refused: a count above 255");
  spit(bad, "FFMBUCKETS 1 8\n2 1 65536\n");
  check(has(refusal(bad, 8), bad, "outside [0, 65536)"), "refused: an edge that is no bin");
  spit(bad, "FFMBUCKETS 1 8\n2 x\n");
  check(has(refusal(bad, 8), bad, "expected"), "refused: a line that is not numbers");
  bool threw = false;
  try {
    ftrl::ValueBuckets m = t;
    m.edges[1 * 255 + 1] = 0;  // (field 1: 0, 0, 65535)
    ftrl::write_value_buckets(bad, m);
  } catch (const std::invalid_argument &) {
    threw = true;
  }
  check(threw, "write refuses edges that do not ascend");
  std::printf("%d ok, %d failed\n", n_ok, n_fail);
  return n_fail == 0 ? 0 : 1;
}
