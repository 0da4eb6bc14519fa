// Stand-alone check of --min_count / --rare_bits / --rare_ids / --rare_ids_out in host/cmd_option.cpp (no GPU, no
// engine library): the defaults, what is accepted, and every refusal -- all of them made while the options are
// parsed, before a device is opened.  Built and run by tests/test_rare_ids_host.py, once plainly and once under
// -fsanitize=address,undefined.
//   usage: rare_option <libffm file>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../ftrl-ffm_amd/host/cmd_option.h"

static int n_ok = 0, n_fail = 0;
static void check(bool cond, const char *what) {
  std::printf("%s  %s\n", cond ? "ok  " : "FAIL", what);
  (cond ? n_ok : n_fail)++;
}

static std::string g_data;

static config_options parse(std::vector<std::string> extra, bool with_train = true) {
  std::vector<std::string> args = {"prog"};
  if (with_train) args.insert(args.end(), {"--train_data", g_data});
  else args.insert(args.end(), {"--predict_data", g_data, "--predict_out", "p.txt"});  // (a run that only scores)
  args.insert(args.end(), extra.begin(), extra.end());
  std::vector<char *> argv;
  for (auto &a : args) argv.push_back(a.data());
  config_options opt;
  opt.parse_option(static_cast<int>(argv.size()), argv.data());
  return opt;
}
// The message the options are refused with; "" when they parse.
static std::string refusal(std::vector<std::string> extra, bool with_train = true) {
  try {
    parse(std::move(extra), with_train);
  } catch (const std::invalid_argument &e) {
    return e.what();
  }
  return "";
}
static bool has(const std::string &msg, const char *part) { return msg.find(part) != std::string::npos; }

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  g_data = argv[1];
  using V = std::vector<std::string>;
  const V hashed = {"--hash_feats", "true"};
  auto with = [&](V more) {
    V all = hashed;
    all.insert(all.end(), more.begin(), more.end());
    return all;
  };
  {
    const config_options d = parse({});
    check(d.min_count == 0 && d.rare_bits == 0 && d.rare_ids.empty() && d.rare_ids_out.empty() && d.rare_words.empty() && d.rare_map_bits == 0,
          "the defaults: no fold");
  }
  {
    const config_options o = parse(with({"--min_count", "10", "--rare_bits", "20", "--rare_ids_out", "m.rare"}));
    check(o.min_count == 10 && o.rare_bits == 20 && o.rare_ids_out == "m.rare", "--min_count 10 --rare_bits 20 --rare_ids_out m.rare");
  }
  check(refusal({"--min_count", "0"}).empty() && refusal({"--min_count", "1"}).empty() && refusal({"--min_count", "1", "--n_gpus", "1"}).empty(),
        "--min_count 0 and 1 are off: nothing else is asked of the run");
  check(parse(with({"--rare_ids", "@m.rare"})).rare_ids == "@m.rare", "--rare_ids @FILE");
  check(refusal(with({"--rare_ids", "@m.rare", "--resume_from", "ck", "--n_epochs", "0"}), false).empty(),
        "--rare_ids @FILE goes with --resume_from and needs no --train_data");
  check(has(refusal({"--min_count", "3"}), "it needs --hash_feats true") && has(refusal({"--min_count", "3", "--hash_feats", "false"}), "--hash_feats true"),
        "refused: --min_count > 1 without --hash_feats true");
  check(has(refusal({"--rare_ids", "@m.rare"}), "it needs --hash_feats true"), "refused: --rare_ids without --hash_feats true");
  check(has(refusal(with({"--min_count", "3", "--n_gpus", "2", "--field_ranges", "uniform"})), "--n_gpus > 1 is not allowed with it"),
        "refused: --min_count with --n_gpus > 1");
  check(has(refusal(with({"--rare_ids", "@m.rare", "--n_gpus", "2", "--field_ranges", "uniform"})), "--n_gpus > 1 is not allowed with it"),
        "refused: --rare_ids with --n_gpus > 1");
  {
    const std::string msg = refusal(with({"--min_count", "3", "--resume_from", "ck"}));
    check(has(msg, "is not allowed with --resume_from") && has(msg, "--rare_ids @FILE"), "refused: --min_count > 1 with --resume_from");
  }
  check(has(refusal(with({"--min_count", "3", "--n_epochs", "0"}), false), "it needs --train_data"), "refused: --min_count > 1 without --train_data");
  check(has(refusal(with({"--min_count", "3", "--rare_ids", "@m.rare"})), "give one of the two"), "refused: both --min_count and --rare_ids");
  check(has(refusal(with({"--rare_ids", "m.rare"})), "takes @FILE") && has(refusal(with({"--rare_ids", "@"})), "takes @FILE"),
        "refused: --rare_ids without the @ or without a name");
  check(has(refusal({"--min_count", "-1"}), "[0, 65535]") && has(refusal({"--min_count", "65536"}), "[0, 65535]") &&
            has(refusal({"--min_count", "ten"}), "takes an integer") && has(refusal({"--rare_bits", "7"}), "[8, 30]") &&
            has(refusal({"--rare_bits", "31"}), "[8, 30]") && has(refusal({"--rare_bits", "2x"}), "takes an integer"),
        "refused: values outside their ranges");
  check(has(refusal(with({"--rare_ids_out", "m.rare"})), "it needs --min_count > 1 or --rare_ids @FILE") &&
            has(refusal(with({"--rare_ids_out", "m.rare", "--min_count", "1"})), "it needs --min_count > 1"),
        "refused: --rare_ids_out with no map to write");
  check(std::string(cmd_help).find("--min_count <T>") != std::string::npos && std::string(cmd_help).find("--rare_bits <B>") != std::string::npos &&
            std::string(cmd_help).find("--rare_ids_out <file>") != std::string::npos && std::string(cmd_help).find("--rare_ids <@file>") != std::string::npos,
        "the help names the four flags");
  std::printf("%d ok, %d failed\n", n_ok, n_fail);
  return n_fail == 0 ? 0 : 1;
}
