// pair_mask_file_main.cpp -- host/pair_mask.{h,cpp} alone, no engine and no device (tests/test_pair_mask_host.py
// builds this with g++, once plain and once with -fsanitize=address,undefined):
//   round trips of the mask file for n_fields 1, 39 and 64 with 0, 1 and V pairs kept;
//   every rejection the reader promises, each with the path in its message;
//   the selection rule on the tables of argv[2] (per case three lines: `n_fields n_keep`, the V + 1 loss sums, the
//   expected pairs flattened or `refused`), which the test wrote from ftrl_ffm_amd.pair_mask_top.
// usage: pair_mask_file <work dir> <tables>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../ftrl-ffm_amd/host/pair_mask.h"

static int failed = 0;
static void expect(bool ok, const std::string &what) {
  if (!ok) {
    failed++;
    std::printf("FAILED %s\n", what.c_str());
  }
}

static void put(const std::string &path, const std::string &text) {
  std::ofstream out(path);
  out << text;
}

static ftrl::PairList all_pairs(int F) {
  ftrl::PairList p;
  for (int f = 0; f < F; f++)
    for (int g = f; g < F; g++) p.emplace_back(f, g);
  return p;
}

static void round_trips(const std::string &dir) {
  for (int F : {1, 39, 64}) {
    const ftrl::PairList all = all_pairs(F);
    const ftrl::PairList cases[3] = {{}, {all[all.size() / 2]}, all};
    for (const ftrl::PairList &kept : cases) {
      const std::string path = dir + "/mask_" + std::to_string(F) + "_" + std::to_string(kept.size());
      ftrl::write_pair_mask(path, F, kept);
      const ftrl::PairList back = ftrl::read_pair_mask(path, F);
      expect(back == kept, "round trip " + path);
      const std::vector<uint64_t> words = ftrl::pair_mask_words(F, back);
      size_t bits = 0, diagonal = 0;
      bool symmetric = words.size() == static_cast<size_t>(F);
      for (int f = 0; f < F && symmetric; f++)
        for (int g = 0; g < F; g++) {
          const bool a = (words[f] >> g) & 1, b = (words[g] >> f) & 1;
          symmetric = symmetric && a == b;
          bits += a;
          diagonal += a && f == g;
        }
      expect(symmetric && (bits + diagonal) / 2 == kept.size(), "words of " + path);
      std::printf("round trip n_fields %d kept %zu\n", F, kept.size());
    }
  }
}

static void reject(const std::string &dir, const std::string &name, const std::string &text, int F, const std::string &needle) {
  const std::string path = dir + "/" + name;
  if (name != "missing") put(path, text);
  try {
    ftrl::read_pair_mask(path, F);
    expect(false, "reject " + name + ": accepted");
  } catch (const std::invalid_argument &e) {
    const std::string msg = e.what();
    expect(msg.find(path) != std::string::npos, "reject " + name + ": the path is not in `" + msg + "`");
    expect(msg.find(needle) != std::string::npos, "reject " + name + ": `" + needle + "` is not in `" + msg + "`");
  }
  std::printf("reject %s\n", name.c_str());
}

static void rejections(const std::string &dir) {
  reject(dir, "missing", "", 4, "cannot be opened");
  reject(dir, "empty", "", 4, "empty file");
  reject(dir, "magic", "ffm-rare-ids 1 4 0\n", 4, "not a pair mask file");
  reject(dir, "version", "ffm-pair-mask 2 4 0\n", 4, "version 2");
  reject(dir, "header_short", "ffm-pair-mask 1 4\n", 4, "expected");
  reject(dir, "header_text", "ffm-pair-mask 1 four 0\n", 4, "not a number");
  reject(dir, "fields", "ffm-pair-mask 1 5 0\n", 4, "n_fields = 4");
  reject(dir, "count_beyond_v", "ffm-pair-mask 1 4 11\n", 4, "11 pairs kept");
  reject(dir, "count_short", "ffm-pair-mask 1 4 2\n0 1\n", 4, "the header counts 2");
  reject(dir, "count_long", "ffm-pair-mask 1 4 1\n0 1\n0 2\n", 4, "more pairs than");
  reject(dir, "range_f", "ffm-pair-mask 1 4 1\n4 4\n", 4, "outside [0, 4)");
  reject(dir, "range_g", "ffm-pair-mask 1 4 1\n0 4\n", 4, "outside [0, 4)");
  reject(dir, "negative", "ffm-pair-mask 1 4 1\n-1 2\n", 4, "not a number");
  reject(dir, "f_above_g", "ffm-pair-mask 1 4 1\n2 1\n", 4, "f <= g");
  reject(dir, "order", "ffm-pair-mask 1 4 2\n1 1\n0 3\n", 4, "out of order");
  reject(dir, "duplicate", "ffm-pair-mask 1 4 2\n0 3\n0 3\n", 4, "listed twice");
  reject(dir, "three_tokens", "ffm-pair-mask 1 4 1\n0 3 1\n", 4, "`f g` expected");
  reject(dir, "one_token", "ffm-pair-mask 1 4 1\n3\n", 4, "`f g` expected");
  // what the writer refuses, and the words of a pair out of range
  try {
    ftrl::write_pair_mask(dir + "/no/such/dir/mask", 4, {});
    expect(false, "write into a missing directory: accepted");
  } catch (const std::runtime_error &) {}
  try {
    ftrl::pair_mask_words(4, {{0, 4}});
    expect(false, "words of (0, 4) at 4 fields: accepted");
  } catch (const std::invalid_argument &) {}
  try {
    ftrl::read_pair_mask(dir + "/magic", 65);
    expect(false, "65 fields: accepted");
  } catch (const std::invalid_argument &) {}
}

static void selections(const std::string &tables) {
  std::ifstream in(tables);
  expect(in.good(), "the tables open");
  std::string l1, l2, l3;
  int n_cases = 0;
  while (std::getline(in, l1) && std::getline(in, l2) && std::getline(in, l3)) {
    int F = 0, n_keep = 0;
    std::istringstream(l1) >> F >> n_keep;
    std::vector<double> loss;
    std::istringstream s2(l2);
    for (std::string t; s2 >> t;) loss.push_back(std::stod(t));  // (stod reads nan and inf)
    const std::string what = "selection case " + std::to_string(n_cases) + " (n_fields " + std::to_string(F) + ", keep " + std::to_string(n_keep) + ")";
    if (l3.rfind("refused", 0) == 0) {
      try {
        ftrl::select_pairs(F, loss, n_keep);
        expect(false, what + ": accepted");
      } catch (const std::runtime_error &e) {
        expect(l3 == std::string("refused ") + e.what(), what + ": `" + e.what() + "` for `" + l3 + "`");
      } catch (const std::invalid_argument &) {
        expect(l3 == "refused", what + ": an invalid argument for `" + l3 + "`");
      }
    } else {
      ftrl::PairList want;
      std::istringstream s3(l3);
      for (int f, g; s3 >> f >> g;) want.emplace_back(f, g);
      double smallest = -1.0;
      const ftrl::PairList got = ftrl::select_pairs(F, loss, n_keep, &smallest);
      expect(got == want, what);
      double least = 0.0;  // the smallest delta among the kept, computed here
      for (size_t i = 0; i < got.size(); i++) {
        const double d = loss[static_cast<size_t>(got[i].first * F - got[i].first * (got[i].first - 1) / 2 + (got[i].second - got[i].first))] - loss.back();
        if (i == 0 || d < least) least = d;
      }
      expect(smallest == least, what + ": smallest kept delta");
    }
    n_cases++;
    std::printf("selection %d\n", n_cases);
  }
  expect(n_cases > 0, "the tables hold cases");
}

int main(int argc, char **argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s <work dir> <tables>\n", argv[0]);
    return 2;
  }
  try {
    round_trips(argv[1]);
    rejections(argv[1]);
    selections(argv[2]);
  } catch (const std::exception &e) {
    failed++;
    std::printf("FAILED with an exception: %s\n", e.what());
  }
  std::printf("%d failed\n", failed);
  return failed ? 1 : 0;
}
