// Stand-alone check of --normalize_rows in host/cmd_option.cpp (no GPU, no engine library): the default, what is
// accepted, and the --n_gpus refusal -- made while the options are parsed, before a device is opened.  Built and
// run by tests/test_row_norm_host.py, once plainly and once under -fsanitize=address,undefined.
//   usage: row_norm_option <libffm file>
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
  check(!parse({}).normalize_rows, "the default: off");
  check(parse({"--normalize_rows", "true"}).normalize_rows && parse({"--normalize_rows", "1"}).normalize_rows &&
            parse({"--normalize_rows", "True"}).normalize_rows,
        "--normalize_rows true / 1 / True");
  check(!parse({"--normalize_rows", "false"}).normalize_rows && !parse({"--normalize_rows", "0"}).normalize_rows, "--normalize_rows false / 0");
  check(parse({"--normalize_rows", "true", "--model_type", "LR"}).normalize_rows && parse({"--normalize_rows", "true", "--model_type", "FM"}).normalize_rows &&
            parse({"--normalize_rows", "true", "--model_type", "FFM", "--hash_feats", "true"}).normalize_rows,
        "LR, FM, FFM and --hash_feats take it");
  check(refusal({"--normalize_rows", "true", "--resume_from", "ck", "--n_epochs", "0", "--serve_weights", "f32", "--model_type", "FFM"}, false).empty(),
        "goes with --resume_from ck --n_epochs 0 --serve_weights f32 and needs no --train_data");
  {
    const std::string msg = refusal({"--normalize_rows", "true", "--model_type", "FFM", "--n_gpus", "2", "--field_ranges", "uniform"});
    check(has(msg, "--normalize_rows true") && has(msg, "--n_gpus > 1 is not allowed with it") && has(msg, "a shard does not own"),
          "refused: --n_gpus > 1");
  }
  check(refusal({"--normalize_rows", "false", "--model_type", "FFM", "--n_gpus", "2", "--field_ranges", "uniform"}).empty(),
        "--normalize_rows false leaves --n_gpus 2 alone");
  check(std::string(cmd_help).find("--normalize_rows <bool>") != std::string::npos &&
            std::string(cmd_help).find("normalized rows: R scaled") != std::string::npos,
        "the help names the flag and its line");
  std::printf("%d ok, %d failed\n", n_ok, n_fail);
  return n_fail == 0 ? 0 : 1;
}
