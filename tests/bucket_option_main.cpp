// Stand-alone check of --bucket_fields / --n_buckets / --buckets / --buckets_out in host/cmd_option.cpp (no GPU, no
// engine library): the defaults, what is accepted, and every refusal -- all of them made while the options are
// parsed, before a device is opened.  Built and run by tests/test_value_buckets_host.py, once plainly and once under
// -fsanitize=address,undefined.
//   usage: bucket_option <libffm file>
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
  std::vector<std::string> args = {"prog", "--n_fields", "8"};
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
  const V hashed = {"--hash_feats", "true", "--model_type", "FFM"};
  auto with = [&](V more) {
    V all = hashed;
    all.insert(all.end(), more.begin(), more.end());
    return all;
  };
  {
    const config_options d = parse({});
    check(d.bucket_fields.empty() && d.buckets.empty() && d.buckets_out.empty() && d.n_buckets == 32 && d.bucket_field_list.empty() &&
              d.bucket_n_edges.empty() && d.bucket_edges.empty(),
          "the defaults: no table, 32 buckets");
  }
  {
    const config_options o = parse(with({"--bucket_fields", "0-2,7,5-5", "--n_buckets", "16", "--buckets_out", "b.txt"}));
    check(o.bucket_field_list == std::vector<int>({0, 1, 2, 5, 7}) && o.n_buckets == 16 && o.buckets_out == "b.txt",
          "--bucket_fields 0-2,7,5-5 --n_buckets 16 --buckets_out b.txt");
    check(parse(with({"--bucket_fields", "7,7,0-7"})).bucket_field_list == std::vector<int>({0, 1, 2, 3, 4, 5, 6, 7}), "repeats in the list count once");
  }
  check(parse(with({"--buckets", "@b.txt"})).buckets == "@b.txt", "--buckets @FILE");
  check(refusal(with({"--buckets", "@b.txt", "--resume_from", "ck", "--n_epochs", "0"}), false).empty(),
        "--buckets @FILE goes with --resume_from and needs no --train_data");
  check(has(refusal({"--model_type", "FFM", "--bucket_fields", "7"}), "it needs --hash_feats true") &&
            has(refusal({"--model_type", "FFM", "--bucket_fields", "7", "--hash_feats", "false"}), "--hash_feats true"),
        "refused: --bucket_fields without --hash_feats true");
  check(has(refusal({"--model_type", "FFM", "--buckets", "@b.txt"}), "it needs --hash_feats true"), "refused: --buckets without --hash_feats true");
  check(has(refusal({"--hash_feats", "true", "--model_type", "LR", "--bucket_fields", "7"}), "only FFM rows have") &&
            has(refusal({"--hash_feats", "true", "--model_type", "FM", "--buckets", "@b.txt"}), "only FFM rows have"),
        "refused: LR / FM");
  check(has(refusal(with({"--bucket_fields", "7", "--n_gpus", "2", "--field_ranges", "uniform"})), "--n_gpus > 1 is not allowed with it") &&
            has(refusal(with({"--buckets", "@b.txt", "--n_gpus", "2", "--field_ranges", "uniform"})), "--n_gpus > 1 is not allowed with it"),
        "refused: --n_gpus > 1");
  check(has(refusal(with({"--bucket_fields", "7", "--buckets", "@b.txt"})), "give one of the two"), "refused: both flags together");
  {
    const std::string msg = refusal(with({"--bucket_fields", "7", "--resume_from", "ck"}));
    check(has(msg, "is not allowed with --resume_from") && has(msg, "--buckets @FILE"), "refused: --bucket_fields with --resume_from");
  }
  check(has(refusal(with({"--bucket_fields", "7", "--n_epochs", "0"}), false), "it needs --train_data"), "refused: --bucket_fields without --train_data");
  check(has(refusal(with({"--bucket_fields", "8"})), "field 8") && has(refusal(with({"--bucket_fields", "8"})), "--n_fields is 8") &&
            has(refusal(with({"--bucket_fields", "0-12"})), "field 12") && has(refusal(with({"--bucket_fields", "3,999999999"})), "not a field"),
        "refused: a field outside [0, n_fields)");
  check(has(refusal(with({"--bucket_fields", "-1"})), "takes a list") && has(refusal(with({"--bucket_fields", "1,"})), "takes a list") &&
            has(refusal(with({"--bucket_fields", "3-1"})), "takes a list") && has(refusal(with({"--bucket_fields", "a"})), "takes a list") &&
            has(refusal(with({"--bucket_fields", "1;2"})), "takes a list") && has(refusal(with({"--bucket_fields", "12345678901"})), "takes a list"),
        "refused: a list that is not one");
  check(has(refusal({"--n_buckets", "1"}), "[2, 256]") && has(refusal({"--n_buckets", "257"}), "[2, 256]") && has(refusal({"--n_buckets", "-4"}), "[2, 256]") &&
            has(refusal({"--n_buckets", "16x"}), "[2, 256]") && refusal({"--n_buckets", "2"}).empty() && refusal({"--n_buckets", "256"}).empty(),
        "refused: --n_buckets outside [2, 256]");
  check(has(refusal(with({"--buckets", "b.txt"})), "takes @FILE") && has(refusal(with({"--buckets", "@"})), "takes @FILE"),
        "refused: --buckets without the @ or without a name");
  check(has(refusal(with({"--buckets_out", "b.txt"})), "it needs --bucket_fields or --buckets @FILE"), "refused: --buckets_out with no table to write");
  check(std::string(cmd_help).find("--bucket_fields <list>") != std::string::npos && std::string(cmd_help).find("--n_buckets <B>") != std::string::npos &&
            std::string(cmd_help).find("--buckets_out <file>") != std::string::npos && std::string(cmd_help).find("--buckets <@file>") != std::string::npos,
        "the help names the four flags");
  std::printf("%d ok, %d failed\n", n_ok, n_fail);
  return n_fail == 0 ? 0 : 1;
}
