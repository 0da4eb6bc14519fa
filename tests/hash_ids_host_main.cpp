// Stand-alone check of the host side of --hash_feats (no GPU, no engine library): csrc/hash_ids.h -- the
// function the device kernels share -- on the known answers and the edges of its domain, and the flag's
// parsing in host/cmd_option.cpp.  Built and run by tests/test_hash_ids_host.py, once plainly and once
// under -fsanitize=address,undefined.
//   usage: hash_ids_host <libffm file>
#include <climits>
#include <cstdio>
#include <string>
#include <vector>

#include "../ftrl-ffm_amd/csrc/hash_ids.h"
#include "../ftrl-ffm_amd/host/cmd_option.h"

static int n_ok = 0, n_fail = 0;
static void check(bool cond, const char *what) {
  std::printf("%s  %s\n", cond ? "ok  " : "FAIL", what);
  (cond ? n_ok : n_fail)++;
}

static config_options parse(const std::string &data, std::vector<std::string> extra) {
  std::vector<std::string> args = {"prog", "--train_data", data};
  args.insert(args.end(), extra.begin(), extra.end());
  std::vector<char *> argv;
  for (auto &a : args) argv.push_back(a.data());
  config_options opt;
  opt.parse_option(static_cast<int>(argv.size()), argv.data());
  return opt;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  using ftrl_hash::Map;
  const Map one{nullptr, 846153, 39, 1};
  check(ftrl_hash::hash_entry(one, 0, 0) == 485182, "known answer (0, 0)");
  check(ftrl_hash::hash_entry(one, 3, 12345) == 487208, "known answer (3, 12345)");
  check(ftrl_hash::hash_entry(one, 38, INT_MAX) == 441169, "known answer (38, INT32_MAX)");
  check(ftrl_hash::hash_entry(one, 0, 1) == 181360, "known answer (0, 1)");
  check(ftrl_hash::hash_entry(one, 0, -1) == -1 && ftrl_hash::hash_entry(one, 0, INT_MIN) == -1, "negative ids stay erased");
  check(ftrl_hash::hash_entry(one, -1, 5) == -1 && ftrl_hash::hash_entry(one, 39, 5) == -1 &&
            ftrl_hash::hash_entry(one, INT_MAX, 5) == -1 && ftrl_hash::hash_entry(one, INT_MIN, 5) == -1,
        "fields outside [0, n_fields) erase their entry");
  const int32_t start[6] = {0, 7, 8, 108, 150, 203};
  const Map ranges{start, 203, 5, 1};
  bool inside = true, width1 = true;
  for (int f = 0; f < 5; f++)
    for (int64_t id = 0; id <= INT_MAX; id += 9999991) {
      const int32_t h = ftrl_hash::hash_entry(ranges, f, static_cast<int32_t>(id));
      inside = inside && h >= start[f] && h < start[f + 1];
      if (f == 1) width1 = width1 && h == 7;
    }
  check(inside, "every id lands in its field's range");
  check(width1, "a field of width 1 maps everything to lo");
  const Map flat{nullptr, 203, 1, 0};  // LR / FM: the field is not looked at, not even a wild one
  check(ftrl_hash::hash_entry(flat, INT_MAX, 77) == ftrl_hash::hash_entry(flat, 0, 77) &&
            ftrl_hash::hash_entry(flat, -5, 77) == ftrl_hash::hash_into(0, 77, 0, 203u),
        "LR / FM take the field as 0");
  check(ftrl_hash::hash_into(INT_MAX, INT_MAX, 0, 0x7fffffffu) >= 0, "the widest range and the largest field wrap, never overflow");
  const std::string data = argv[1];
  check(!parse(data, {}).hash_feats, "--hash_feats defaults to false");
  check(parse(data, {"--hash_feats", "true"}).hash_feats && parse(data, {"--hash_feats", "1"}).hash_feats, "--hash_feats true / 1");
  check(!parse(data, {"--hash_feats", "false"}).hash_feats, "--hash_feats false");
  check(std::string(cmd_help).find("--hash_feats <bool>") != std::string::npos, "the help names the flag");
  std::printf("%d ok, %d failed\n", n_ok, n_fail);
  return n_fail == 0 ? 0 : 1;
}
