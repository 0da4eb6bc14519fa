// Stand-alone check of --device_parse in host/cmd_option.cpp (no GPU, no engine library): the default, what is
// accepted, and the two refusals -- made while the options are parsed, before a device is opened.  Built and run by
// tests/test_text_parse_host.py, once plainly and once under -fsanitize=address,undefined.
//   usage: device_parse_option <libffm file>
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

static config_options parse(std::vector<std::string> extra) {
  std::vector<std::string> args = {"prog", "--n_fields", "8", "--model_type", "FFM", "--train_data", g_data};
  args.insert(args.end(), extra.begin(), extra.end());
  std::vector<char *> argv;
  for (auto &a : args) argv.push_back(a.data());
  config_options opt;
  opt.parse_option(static_cast<int>(argv.size()), argv.data());
  return opt;
}
// The message the options are refused with; "" when they parse.
static std::string refusal(std::vector<std::string> extra) {
  try {
    parse(std::move(extra));
  } catch (const std::invalid_argument &e) {
    return e.what();
  }
  return "";
}
static bool has(const std::string &msg, const char *part) { return msg.find(part) != std::string::npos; }

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  g_data = argv[1];
  check(!parse({}).device_parse, "the default: off");
  check(parse({"--device_parse", "true", "--hash_feats", "true", "--min_count", "3"}).device_parse, "with --min_count 3");
  check(parse({"--device_parse", "1", "--hash_feats", "true", "--bucket_fields", "0-1"}).device_parse, "with --bucket_fields 0-1");
  check(parse({"--device_parse", "True", "--field_ranges", "counted"}).device_parse, "with --field_ranges counted");
  check(!parse({"--device_parse", "false"}).device_parse && !parse({"--device_parse", "0", "--cmd", "true"}).device_parse,
        "--device_parse false asks for nothing");
  {
    const std::string msg = refusal({"--device_parse", "true"});
    check(has(msg, "--device_parse true") && has(msg, "--min_count > 1") && has(msg, "--bucket_fields") && has(msg, "--field_ranges counted"),
          "refused: none of the three passes");
    check(!refusal({"--device_parse", "true", "--hash_feats", "true", "--min_count", "1"}).empty() &&
              !refusal({"--device_parse", "true", "--field_ranges", "uniform"}).empty(),
          "refused: --min_count 1 and --field_ranges uniform are no pass");
  }
  {
    const std::string msg = refusal({"--device_parse", "true", "--field_ranges", "counted", "--cmd", "true"});
    check(has(msg, "--device_parse true") && has(msg, "--cmd"), "refused: --cmd true");
  }
  check(std::string(cmd_help).find("--device_parse <bool>") != std::string::npos &&
            std::string(cmd_help).find("device parse: C chunks, B bytes, H parsed by the host (first at byte N)") != std::string::npos,
        "the help names the flag and its line");
  std::printf("%d ok, %d failed\n", n_ok, n_fail);
  return n_fail == 0 ? 0 : 1;
}
