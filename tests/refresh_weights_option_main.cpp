// Stand-alone check of host/cmd_option.cpp's --refresh_weights: default, spellings, the flag among others,
// a missing value, the help text.  argv[1]: a libffm file (parse_option looks at the training file's format).
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

static config_options parse(const std::string &data, std::vector<std::string> extra) {
  std::vector<std::string> args = {"prog", "--train_data", data, "--model_type", "FFM"};
  args.insert(args.end(), extra.begin(), extra.end());
  std::vector<char *> argv;
  for (auto &a : args) argv.push_back(a.data());
  config_options o;
  o.parse_option(static_cast<int>(argv.size()), argv.data());
  return o;
}

int main(int argc, char *argv[]) {
  if (argc != 2) return 2;
  const std::string data = argv[1];
  expect(!config_options().refresh_weights, "default-constructed options: off");
  expect(!parse(data, {}).refresh_weights, "not given: off");
  expect(parse(data, {"--refresh_weights", "true"}).refresh_weights, "true");
  expect(parse(data, {"--refresh_weights", "True"}).refresh_weights, "True");
  expect(parse(data, {"--refresh_weights", "1"}).refresh_weights, "1");
  expect(!parse(data, {"--refresh_weights", "false"}).refresh_weights, "false");
  expect(!parse(data, {"--refresh_weights", "0"}).refresh_weights, "0");
  expect(!parse(data, {"--refresh_weights", "yes"}).refresh_weights, "anything else is false, as for --learn");
  {
    const config_options o = parse(data, {"--learn", "true", "--refresh_weights", "true", "--n_gpus", "2", "--n_epochs", "0"});
    expect(o.refresh_weights && o.learn && o.n_gpus == 2 && o.epoch == 0, "beside --learn, --n_gpus and --n_epochs 0");
  }
  expect(parse(data, {"--refresh_weights", "true", "--refresh_weights", "false"}).refresh_weights == false, "the last one wins");
  bool threw = false;
  try { parse(data, {"--refresh_weights"}); } catch (const std::invalid_argument &) { threw = true; }
  expect(threw, "without a value: invalid_argument");
  const std::string help(cmd_help);
  expect(help.find("--refresh_weights <bool>") != std::string::npos && help.find("default:false") != std::string::npos,
         "the help text names the flag");
  expect(help.find("epoch N weights: linear L live, Z nonzero, M moved; latent L live, Z nonzero, M moved") != std::string::npos,
         "the help text shows the line");
  std::printf("%d failed\n", failed);
  return failed ? 1 : 0;
}
