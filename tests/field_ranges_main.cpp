// Stand-alone check of the CLI's --field_ranges forms (host/cmd_option.cpp) and of the ranges file
// (host/field_ranges.cpp): the accepted spellings, every refusal with its message, the reader's file:line errors,
// a write / read round trip, the help text.  argv[1]: a libffm file (parse_option looks at the file's format);
// argv[2]: a directory to write into.
#include <cstdio>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../ftrl-ffm_amd/host/cmd_option.h"
#include "../ftrl-ffm_amd/host/field_ranges.h"

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
static bool has(const std::string &s, const std::string &part) { return s.find(part) != std::string::npos; }

static std::string dir;
static std::string file_with(const char *name, const std::string &text) {
  const std::string path = dir + "/" + name;
  std::ofstream(path) << text;
  return path;
}
// the message read_field_ranges refuses a file of `text` with (3 fields, 100 features), or "" when it reads it
static std::string read_refusal(const std::string &text, bool hashed = true) {
  const std::string path = file_with("r.txt", text);
  try { ftrl::read_field_ranges(path, 3, 100, hashed); } catch (const std::invalid_argument &e) {
    const std::string msg = e.what();
    return msg.compare(0, path.size() + 1, path + ":") == 0 ? msg.substr(path.size()) : "no file prefix: " + msg;
  }
  return "";
}

int main(int argc, char *argv[]) {
  if (argc != 3) return 2;
  const std::string data = argv[1];
  dir = argv[2];
  using V = std::vector<std::string>;
  const V train = {"--model_type", "FFM", "--train_data", data};
  auto with = [&](V extra) { V a = train; a.insert(a.end(), extra.begin(), extra.end()); return a; };

  // ---- the spellings
  expect(config_options().field_ranges == "none" && config_options().field_start.empty() && config_options().field_ranges_out.empty(),
         "default-constructed options: none, no ranges, no output file");
  expect(parse(train).field_ranges == "none", "not given: none");
  expect(parse(with({"--field_ranges", "uniform"})).field_ranges == "uniform", "uniform");
  expect(parse(with({"--field_ranges", "none"})).field_ranges == "none", "none");
  expect(parse(with({"--field_ranges", "sometimes"})).field_ranges == "sometimes", "any other spelling is taken as it always was");
  expect(parse(with({"--field_ranges", "counted"})).field_ranges == "counted", "counted with a training file");
  expect(parse(with({"--field_ranges", "counted", "--hash_feats", "true", "--field_ranges_out", "r.txt"})).field_ranges_out == "r.txt",
         "counted with --hash_feats and --field_ranges_out");
  expect(parse(with({"--field_ranges", "@r.txt"})).field_ranges == "@r.txt", "@FILE");
  expect(parse(with({"--field_ranges", "uniform", "--field_ranges_out", "u.txt"})).field_ranges_out == "u.txt", "uniform with --field_ranges_out");
  expect(parse(with({"--field_ranges", "@r.txt", "--field_ranges_out", "u.txt"})).field_ranges_out == "u.txt", "@FILE with --field_ranges_out");
  expect(parse(with({"--field_ranges", "counted"})).field_start.empty(), "parsing resolves nothing: no ranges yet");
  {
    const config_options o = parse({"--model_type", "FFM", "--resume_from", "ck", "--n_epochs", "0", "--predict_data", data, "--predict_out",
                                    "p.txt", "--field_ranges", "@r.txt", "--serve_weights", "f16", "--hash_feats", "true"});
    expect(o.field_ranges == "@r.txt" && o.serve_weights == "f16", "@FILE beside --resume_from ck --n_epochs 0 and --serve_weights");
  }
  expect(parse(with({"--field_ranges", "@r.txt", "--n_gpus", "2"})).n_gpus == 2, "@FILE with --n_gpus 2 parses (the model demands uniform)");

  // ---- the refusals of counted
  expect(has(refusal({"--model_type", "FFM", "--field_ranges", "counted", "--n_epochs", "0", "--predict_data", data, "--predict_out", "p"}),
             "--field_ranges counted counts the ids of the training file: it needs --train_data"), "counted without --train_data");
  {
    const std::string msg = refusal(with({"--field_ranges", "counted", "--resume_from", "ck"}));
    expect(has(msg, "--field_ranges counted is not allowed with --resume_from") && has(msg, "--field_ranges @FILE"),
           "counted with --resume_from points to @FILE");
  }
  expect(has(refusal(with({"--field_ranges", "counted", "--n_gpus", "2"})), "--n_gpus > 1 is not allowed with it"), "counted with --n_gpus 2");
  expect(refusal(with({"--field_ranges", "counted", "--n_gpus", "1"})).empty(), "counted with --n_gpus 1 is fine");
  {
    V fm = with({"--field_ranges", "counted"});
    fm[1] = "FM";
    expect(has(refusal(fm), "only FFM rows have (got --model_type FM)"), "counted with --model_type FM");
    fm[1] = "lr";
    expect(has(refusal(fm), "only FFM rows have (got --model_type LR)"), "counted with --model_type lr");
  }
  // ---- @FILE and --field_ranges_out
  expect(has(refusal(with({"--field_ranges", "@"})), "needs a file name after the @"), "@ without a file name");
  {
    V fm = with({"--field_ranges", "@r.txt"});
    fm[1] = "FM";
    expect(has(refusal(fm), "only FFM has (got --model_type FM)"), "@FILE with --model_type FM");
  }
  expect(has(refusal(with({"--field_ranges_out", "u.txt"})), "--field_ranges_out writes the fields' id ranges"), "--field_ranges_out with none");
  expect(has(refusal(with({"--field_ranges", "sometimes", "--field_ranges_out", "u.txt"})), "uniform, counted or @FILE"),
         "--field_ranges_out with another spelling");
  expect(has(refusal(with({"--field_ranges_out"})), "exactly one value"), "--field_ranges_out without a value");

  // ---- the ranges file
  expect(read_refusal("0\n10\n40\n100\n").empty(), "a good file");
  expect(read_refusal("0\n\n10\r\n40 \n100").empty(), "blank lines, line ends and a missing last line end");
  {
    const std::vector<int32_t> fs = ftrl::read_field_ranges(file_with("r.txt", "0\n10\n40\n100\n"), 3, 100, true);
    expect(fs == std::vector<int32_t>({0, 10, 40, 100}), "its values");
  }
  expect(has(read_refusal("0\n10\nforty\n100\n"), ":3: not an integer: `forty`"), "a word, with its line");
  expect(has(read_refusal("0\n10\n4 0\n100\n"), ":3: not an integer"), "two numbers on a line");
  expect(has(read_refusal("0\n10\n99999999999999999999\n100\n"), ":3: not an integer"), "a number beyond 64 bits");
  expect(has(read_refusal("1\n10\n40\n100\n"), ":1: the first value must be 0"), "does not start at 0");
  expect(has(read_refusal("0\n40\n10\n100\n"), ":3: the values must ascend: 10 after 40"), "descending");
  expect(has(read_refusal("0\n10\n10\n100\n"), ":3: field 1 has width 0"), "a width of 0 under --hash_feats");
  expect(read_refusal("0\n10\n10\n100\n", false).empty(), "a width of 0 without --hash_feats is a hint like any other");
  expect(has(read_refusal("0\n10\n40\n"), ":3: 3 values, n_fields + 1 = 4 expected"), "too few values");
  expect(has(read_refusal(""), ":0: 0 values"), "an empty file");
  expect(has(read_refusal("0\n10\n40\n100\n100\n"), ":5: more than n_fields + 1 = 4 values"), "too many values");
  expect(has(read_refusal("0\n10\n40\n90\n"), ":4: the last value must be n_feats = 100, got 90"), "does not end at n_feats");
  expect(has(read_refusal("0\n10\n40\n101\n"), ":4: 101 is outside [0, n_feats = 100]"), "beyond n_feats");
  expect(has(read_refusal("0\n-1\n40\n100\n"), ":2: -1 is outside"), "a negative value");
  {
    std::string msg;
    try { ftrl::read_field_ranges(dir + "/not_there.txt", 3, 100, true); } catch (const std::invalid_argument &e) { msg = e.what(); }
    expect(has(msg, "not_there.txt: cannot be opened"), "a missing file");
  }
  {
    const std::vector<int32_t> u = ftrl::uniform_field_ranges(3, 100);
    expect(u == std::vector<int32_t>({0, 33, 66, 100}), "uniform ranges: the last field takes the rest");
    const std::string path = dir + "/u.txt";
    ftrl::write_field_ranges(path, u);
    expect(ftrl::read_field_ranges(path, 3, 100, true) == u, "written ranges read back");
    std::string msg;
    try { ftrl::uniform_field_ranges(8, 7); } catch (const std::invalid_argument &e) { msg = e.what(); }
    expect(has(msg, "needs n_feats >= n_fields"), "uniform ranges of fewer ids than fields");
    msg.clear();
    try { ftrl::write_field_ranges(dir + "/no/such/dir/u.txt", u); } catch (const std::runtime_error &e) { msg = e.what(); }
    expect(has(msg, "cannot write"), "an unwritable path");
  }

  const std::string help(cmd_help);
  expect(has(help, "--field_ranges <uniform|none|counted|@FILE>") && has(help, "--field_ranges_out <path>"), "the help text names both flags");
  expect(has(help, "field f: ~D distinct ids, ids [lo, hi)") &&
             has(help, "field ranges: counted from R rows (E entries, B erased) in T s; ~S distinct ids for N features (load X)"),
         "the help text shows the lines");
  expect(has(help, "not recorded in checkpoints") && has(help, "passes @FILE") && has(help, "--n_gpus > 1 takes uniform only"),
         "the help text says what a resumed run passes and what several GPUs take");
  std::printf("%d failed\n", failed);
  return failed ? 1 : 0;
}
