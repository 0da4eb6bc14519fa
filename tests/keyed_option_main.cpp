// Stand-alone check of host/cmd_option.cpp's --auc_key_field / --auc_key_rows: the defaults, the accepted
// combinations, the five refusals with their messages (all before a device is opened: parse_option touches
// none), the help text.  argv[1]: a libffm file, argv[2]: a libsvm file (parse_option looks at the format).
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../ftrl-ffm_amd/host/cmd_option.h"

static int failed = 0;
static void expect(bool ok, const char *what) {
  std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
  if (!ok) failed++;
}

static config_options parse(std::vector<std::string> args) {
  args.insert(args.begin(), "prog");
  std::vector<char *> argv;
  for (auto &a : args) argv.push_back(a.data());
  config_options o;
  o.parse_option(static_cast<int>(argv.size()), argv.data());
  return o;
}

// the message parse_option refuses `args` with, or "" when it accepts them
static std::string refusal(const std::vector<std::string> &args) {
  try { parse(args); } catch (const std::invalid_argument &e) { return e.what(); }
  return "";
}
static bool has(const std::string &s, const char *part) { return s.find(part) != std::string::npos; }

int main(int argc, char *argv[]) {
  if (argc != 3) return 2;
  const std::string ffm = argv[1], svm = argv[2];
  using V = std::vector<std::string>;
  const V train = {"--model_type", "FFM", "--train_data", ffm, "--eval_data", ffm, "--metrics", "auc"};
  auto with = [&](V extra) { V a = train; a.insert(a.end(), extra.begin(), extra.end()); return a; };

  expect(config_options().auc_key_field == -1 && config_options().auc_key_rows == 16777216, "default-constructed options: off, 2^24 rows");
  expect(parse(train).auc_key_field == -1, "not given: off");
  {
    const config_options o = parse(with({"--auc_key_field", "0"}));
    expect(o.auc_key_field == 0 && o.auc_key_rows == 16777216, "--auc_key_field 0: 2^24 rows by default");
  }
  {
    const config_options o = parse(with({"--auc_key_rows", "1000", "--auc_key_field", "7"}));
    expect(o.auc_key_field == 7 && o.auc_key_rows == 1000, "the last field of the default 8, 1000 rows, in either order");
  }
  expect(parse(with({"--n_fields", "40", "--auc_key_field", "39"})).auc_key_field == 39, "--n_fields before the flag");
  expect(parse(with({"--auc_key_field", "39", "--n_fields", "40"})).auc_key_field == 39, "--n_fields after the flag");
  {
    const config_options o = parse({"--model_type", "FFM", "--resume_from", "ck", "--n_epochs", "0", "--eval_data", ffm, "--train_data", ffm,
                                    "--metrics", "auc", "--auc_key_field", "2", "--serve_weights", "f32"});
    expect(o.auc_key_field == 2 && o.serve_weights == "f32" && o.epoch == 0, "with --resume_from ck --n_epochs 0 --serve_weights f32");
  }
  expect(parse(with({"--auc_key_rows", "5"})).auc_key_field == -1, "--auc_key_rows alone asks for nothing");
  // the five refusals
  expect(has(refusal({"--model_type", "FFM", "--train_data", ffm, "--auc_key_field", "0"}), "it needs --metrics auc"), "without --metrics auc");
  expect(has(refusal({"--model_type", "FFM", "--train_data", ffm, "--metrics", "none", "--auc_key_field", "0"}), "it needs --metrics auc"),
         "with --metrics none");
  expect(has(refusal({"--model_type", "LR", "--train_data", svm, "--metrics", "auc", "--auc_key_field", "0"}),
             "only FFM rows have (got --model_type LR)"), "--model_type LR");
  expect(has(refusal({"--model_type", "fm", "--train_data", svm, "--metrics", "auc", "--auc_key_field", "0"}),
             "only FFM rows have (got --model_type FM)"), "--model_type fm");
  expect(has(refusal(with({"--auc_key_field", "0", "--n_gpus", "2"})), "--n_gpus > 1 is not allowed"), "--n_gpus 2");
  expect(has(refusal(with({"--auc_key_field", "8"})), "is not a field of this model: --n_fields is 8"), "F == n_fields");
  expect(has(refusal(with({"--auc_key_field", "5", "--n_fields", "4"})), "--n_fields is 4"), "F above a smaller --n_fields");
  expect(has(refusal(with({"--auc_key_field", "-1"})), "names a field: >= 0"), "F negative");
  expect(has(refusal(with({"--auc_key_field", "0", "--auc_key_rows", "0"})), "--auc_key_rows must be positive, got 0"), "N == 0");
  expect(has(refusal(with({"--auc_key_field", "0", "--auc_key_rows", "-4"})), "--auc_key_rows must be positive, got -4"), "N negative");
  expect(has(refusal(with({"--auc_key_field", "user"})), "takes an integer"), "not a number");
  expect(has(refusal(with({"--auc_key_rows", "1e6", "--auc_key_field", "0"})), "takes an integer"), "not an integer");
  expect(has(refusal(with({"--auc_key_field"})), "exactly one value"), "without a value");
  // --metrics keeps its text
  expect(has(refusal(with({"--metrics", "gauc"})), "--metrics takes auc or none"), "--metrics takes auc or none, as before");
  const std::string help(cmd_help);
  expect(has(help, "--metrics <auc|none>"), "the --metrics text stays");
  expect(has(help, "--auc_key_field <F>") && has(help, "--auc_key_rows <N>") && has(help, "default:16777216"), "the help text names the flags");
  expect(has(help, "gauc: G (K keys, M mixed, R of T rows; U unkeyed,") && has(help, "FFM only, one GPU"), "the help text shows the line and the limits");
  std::printf("%d failed\n", failed);
  return failed ? 1 : 0;
}
