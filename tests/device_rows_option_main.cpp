// Stand-alone check of --device_rows in host/cmd_option.cpp (no GPU, no engine library): the default, what is
// accepted, and every refusal by the flags its message names -- made while the options are parsed, before a device is
// opened.  The twin of tests/device_parse_option_main.cpp; built and run by tests/test_row_cut_host.py, once plainly
// and once under -fsanitize=address,undefined.
//   usage: device_rows_option <libffm file>
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
  std::vector<std::string> args = {"prog", "--n_fields", "8", "--model_type", "FFM"};
  if (with_train) args.insert(args.end(), {"--train_data", g_data});
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
  const std::string on = "--device_rows true";
  check(!parse({}).device_rows, "the default: off");
  check(parse({"--device_rows", "true"}).device_rows, "online training of --train_data");
  check(parse({"--device_rows", "1", "--n_epochs", "0", "--eval_data", g_data}).device_rows, "--n_epochs 0 with --eval_data");
  check(parse({"--device_rows", "True", "--n_epochs", "0", "--predict_data", g_data, "--predict_out", "p.txt"}, false).device_rows,
        "--n_epochs 0 with --predict_data and no --train_data");
  check(parse({"--device_rows", "true", "--device_parse", "true", "--hash_feats", "true", "--min_count", "3"}).device_rows &&
            parse({"--device_rows", "true", "--device_parse", "true", "--hash_feats", "true", "--min_count", "3"}).device_parse,
        "the two flags combine");
  check(parse({"--device_rows", "true", "--model_type", "FFM", "--metrics", "auc", "--auc_key_field", "0", "--refresh_weights", "true"}).device_rows,
        "with --metrics auc, --auc_key_field and --refresh_weights");
  check(parse({"--device_rows", "true", "--n_epochs", "0", "--eval_data", g_data, "--pos_weight", "2"}).device_rows,
        "sample weights on a run that trains nothing");
  check(!parse({"--device_rows", "false", "--online", "false"}).device_rows && !parse({"--device_rows", "0", "--compact_rows", "true"}).device_rows,
        "--device_rows false asks for nothing");
  {
    const std::string msg = refusal({"--device_rows", "true", "--online", "false"});
    check(has(msg, on.c_str()) && has(msg, "--online false"), "refused: --online false");
  }
  {
    const std::string msg = refusal({"--device_rows", "true", "--cmd", "true"});
    check(has(msg, on.c_str()) && has(msg, "--cmd true"), "refused: --cmd true");
  }
  {
    const std::string msg = refusal({"--device_rows", "true", "--n_gpus", "2", "--field_ranges", "uniform"});
    check(has(msg, on.c_str()) && has(msg, "--n_gpus > 1"), "refused: --n_gpus 2");
  }
  {
    const std::string msg = refusal({"--device_rows", "true", "--compact_rows", "true"});
    check(has(msg, on.c_str()) && has(msg, "--compact_rows true"), "refused: --compact_rows true");
  }
  for (const char *flag : {"--pos_weight", "--neg_weight"}) {
    const std::string msg = refusal({"--device_rows", "true", flag, "2"});
    check(has(msg, on.c_str()) && has(msg, "--pos_weight") && has(msg, "--neg_weight") && has(msg, "--weight_data") && has(msg, "--n_epochs > 0"),
          "refused: a class weight on a run that trains");
  }
  {
    const std::string msg = refusal({"--device_rows", "true", "--weight_data", g_data});
    check(has(msg, on.c_str()) && has(msg, "--weight_data") && has(msg, "--n_epochs > 0"), "refused: --weight_data on a run that trains");
  }
  {
    const std::string msg = refusal({"--device_rows", "true", "--n_epochs", "0"});
    check(has(msg, on.c_str()) && has(msg, "--train_data") && has(msg, "--n_epochs > 0") && has(msg, "--eval_data") && has(msg, "--predict_data"),
          "refused: no file to read (--n_epochs 0, nothing to evaluate or score)");
  }
  {
    // --device_parse keeps its own meaning: the counting passes only
    const std::string msg = refusal({"--device_parse", "true", "--device_rows", "true"});
    check(has(msg, "--device_parse true") && has(msg, "--min_count > 1") && has(msg, "--device_rows true"),
          "--device_parse true still needs a counting pass, and its refusal points here");
  }
  const std::string help(cmd_help);
  check(help.find("--device_rows <bool>") != std::string::npos &&
            help.find("chunks, B bytes, H parsed by the host (first at byte N), K blocks") != std::string::npos &&
            help.find("--field_importance keeps reading --eval_data through the host") != std::string::npos,
        "the help names the flag, its line and what stays on the host parser");
  std::printf("%d ok, %d failed\n", n_ok, n_fail);
  return n_fail == 0 ? 0 : 1;
}
