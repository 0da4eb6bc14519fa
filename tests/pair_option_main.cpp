// Stand-alone check of --pair_importance in host/cmd_option.cpp and of host/importance.cpp (no GPU, no engine
// library): the default, what is accepted, every refusal -- all made while the options are parsed, before a device
// is opened --, the pairs' numbering, the histogram memory and the printed lines of both flags.  Built and run by
// tests/test_pair_ablation_host.py, once plainly and once under -fsanitize=address,undefined.
//   usage: pair_option <libffm file> <libsvm file> <scratch file> [libffm_engine.so: its numbering is compared too]
#include <dlfcn.h>

#include <cstdint>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../ftrl-ffm_amd/host/cmd_option.h"
#include "../ftrl-ffm_amd/host/importance.h"

static int n_ok = 0, n_fail = 0;
static void check(bool cond, const char *what) {
  std::printf("%s  %s\n", cond ? "ok  " : "FAIL", what);
  (cond ? n_ok : n_fail)++;
}

static config_options parse(std::vector<std::string> args) {
  args.insert(args.begin(), "prog");
  std::vector<char *> argv;
  for (auto &a : args) argv.push_back(a.data());
  config_options opt;
  opt.parse_option(static_cast<int>(argv.size()), argv.data());
  return opt;
}
// The message the options are refused with; "" when they parse.
static std::string refusal(std::vector<std::string> args) {
  try {
    parse(std::move(args));
  } catch (const std::invalid_argument &e) {
    return e.what();
  }
  return "";
}
static bool has(const std::string &msg, const char *part) { return msg.find(part) != std::string::npos; }

static std::string printed(const char *path, int n_fields, unsigned long long rows, const std::vector<double> &loss,
                           const std::vector<ffm_metrics> *auc, int *listed,
                           decltype(&ftrl::print_pair_importance) print = ftrl::print_pair_importance) {
  std::FILE *f = std::fopen(path, "w");
  if (!f) return "<cannot open>";
  *listed = print(f, n_fields, rows, loss, auc);
  std::fclose(f);
  std::ifstream in(path);
  std::stringstream s;
  s << in.rdbuf();
  return s.str();
}

int main(int argc, char **argv) {
  if (argc != 4 && argc != 5) return 2;
  const std::string ffm = argv[1], svm = argv[2];
  using V = std::vector<std::string>;
  const V base = {"--model_type", "FFM", "--n_fields", "8", "--train_data", ffm, "--eval_data", ffm};
  auto with = [&](V more) {
    V all = base;
    all.insert(all.end(), more.begin(), more.end());
    return all;
  };
  const char *what = "--pair_importance true ";
  check(!parse(base).pair_importance && !parse(with({"--pair_importance", "false"})).pair_importance, "the default is false");
  check(parse(with({"--pair_importance", "true"})).pair_importance && parse(with({"--pair_importance", "1"})).pair_importance,
        "--pair_importance true / 1");
  {
    const config_options o = parse(with({"--pair_importance", "true", "--field_importance", "true", "--metrics", "auc"}));
    check(o.pair_importance && o.field_importance && o.metrics == "auc", "with --field_importance true and --metrics auc");
  }
  check(refusal({"--model_type", "FFM", "--n_fields", "8", "--eval_data", ffm, "--resume_from", "ck", "--n_epochs", "0", "--predict_data", ffm,
                 "--predict_out", "p.txt", "--pair_importance", "true"}).empty() &&
            refusal({"--model_type", "FFM", "--n_fields", "8", "--eval_data", ffm, "--resume_from", "ck", "--n_epochs", "0", "--predict_data", ffm,
                     "--predict_out", "p.txt", "--serve_weights", "f16", "--pair_importance", "true"}).empty(),
        "--resume_from ck --n_epochs 0, with and without --serve_weights f16");
  {
    const std::string msg = refusal({"--model_type", "FFM", "--n_fields", "8", "--train_data", ffm, "--pair_importance", "true"});
    check(has(msg, what) && has(msg, "it needs --eval_data"), "refused: no --eval_data");
  }
  check(has(refusal({"--model_type", "LR", "--train_data", svm, "--eval_data", svm, "--pair_importance", "true"}), "only FFM rows have") &&
            has(refusal({"--model_type", "FM", "--train_data", svm, "--eval_data", svm, "--pair_importance", "true"}), "only FFM rows have"),
        "refused: LR / FM");
  check(has(refusal(with({"--pair_importance", "true", "--n_gpus", "2", "--field_ranges", "uniform"})), "--n_gpus > 1 is not allowed with it"),
        "refused: --n_gpus > 1");
  {
    const std::string msg = refusal({"--model_type", "FFM", "--n_fields", "65", "--train_data", ffm, "--eval_data", ffm, "--pair_importance", "true"});
    check(has(msg, what) && has(msg, "--n_fields is 65, at most 64"), "refused: --n_fields 65");
    check(refusal({"--model_type", "FFM", "--n_fields", "64", "--train_data", ffm, "--eval_data", ffm, "--pair_importance", "true"}).empty(),
          "--n_fields 64 is accepted");
  }
  check(has(refusal(with({"--pair_importance", "true", "--n_factors", "12"})), "--n_factors must be 4, 8, 16, 32 or 64 (got 12)") &&
            refusal(with({"--pair_importance", "true", "--n_factors", "64"})).empty(),
        "refused: --n_factors 12");
  check(refusal(with({"--n_factors", "12"})).empty() && refusal({"--model_type", "LR", "--train_data", svm}).empty(),
        "none of it without the flag");
  check(std::string(cmd_help).find("--pair_importance <bool>") != std::string::npos, "the help names the flag");

  // ---- host/importance.cpp
  {
    bool ok = true;
    for (int F = 1; F <= 64; F++) {
      int next = 0;
      for (int f = 0; f < F; f++)
        for (int g = f; g < F; g++) ok = ok && ftrl::pair_index(F, f, g) == next++;
      ok = ok && next == ftrl::pair_count(F);
    }
    check(ok && ftrl::pair_count(39) == 780 && ftrl::pair_count(64) == 2080, "pair_index counts the pairs f <= g in order, for 1 .. 64 fields");
  }
  check(ftrl::pair_histogram_bytes(39) == 781ull * 16777224ull && ftrl::pair_histogram_bytes(64) == 2081ull * 16777224ull &&
            ftrl::pair_histogram_bytes(39) / 1000000000ull == 13 && ftrl::pair_histogram_bytes(64) / 1000000000ull == 34,
        "histogram memory: 13 GB at 39 fields, 35 GB at 64");
  {
    // 3 fields: 6 pairs; pairs (0, 1) and (2, 2) moved the sum
    std::vector<double> loss = {4.0, 5.0, 4.0, 4.0, 4.0, 3.5, 4.0};
    int listed = -1;
    const std::string s = printed(argv[3], 3, 8, loss, nullptr, &listed);
    check(listed == 2 &&
              s == "pair importance: 8 rows, loss 0.500000\n"
                   "pair 0 1: without it loss 0.625000 (delta +0.125000)\n"
                   "pair 2 2: without it loss 0.437500 (delta -0.062500)\n"
                   "pair importance: 2 of 6 pairs listed, 4 never changed a row\n",
          "the lines without AUC");
    std::vector<ffm_metrics> auc(7);
    for (size_t v = 0; v < auc.size(); v++) auc[v].auc = 0.75;
    auc[1].auc = 0.5;
    const std::string t = printed(argv[3], 3, 8, loss, &auc, &listed);
    check(listed == 2 && has(t, "pair importance: 8 rows, loss 0.500000, auc 0.750000\n") &&
              has(t, "pair 0 1: without it loss 0.625000 (delta +0.125000), auc 0.500000 (delta -0.250000)\n") &&
              has(t, "pair 2 2: without it loss 0.437500 (delta -0.062500), auc 0.750000 (delta +0.000000)\n"),
          "the lines with AUC");
    loss.pop_back();
    check(ftrl::print_pair_importance(stdout, 3, 8, loss, nullptr) == -1, "a loss vector of the wrong length prints nothing");
    const std::string none = printed(argv[3], 2, 0, {0.0, 0.0, 0.0, 0.0}, nullptr, &listed);
    check(listed == 0 && none == "pair importance: 0 rows, loss 0.000000\npair importance: 0 of 3 pairs listed, 3 never changed a row\n",
          "an empty file");
  }
  {
    // 3 fields; the lines of every field, moved or not
    std::vector<double> loss = {5.0, 4.0, 3.5, 4.0};
    int lines = -1;
    const std::string s = printed(argv[3], 3, 8, loss, nullptr, &lines, ftrl::print_field_importance);
    check(lines == 3 &&
              s == "field importance: 8 rows, loss 0.500000\n"
                   "field 0: without it loss 0.625000 (delta +0.125000)\n"
                   "field 1: without it loss 0.500000 (delta +0.000000)\n"
                   "field 2: without it loss 0.437500 (delta -0.062500)\n",
          "the fields' lines without AUC");
    std::vector<ffm_metrics> auc(4);
    for (size_t v = 0; v < auc.size(); v++) auc[v].auc = 0.75;
    auc[0].auc = 0.5;
    const std::string t = printed(argv[3], 3, 8, loss, &auc, &lines, ftrl::print_field_importance);
    check(lines == 3 &&
              t == "field importance: 8 rows, loss 0.500000, auc 0.750000\n"
                   "field 0: without it loss 0.625000 (delta +0.125000), auc 0.500000 (delta -0.250000)\n"
                   "field 1: without it loss 0.500000 (delta +0.000000), auc 0.750000 (delta +0.000000)\n"
                   "field 2: without it loss 0.437500 (delta -0.062500), auc 0.750000 (delta +0.000000)\n",
          "the fields' lines with AUC");
    auc.pop_back();
    const std::string short_auc = printed(argv[3], 3, 8, loss, &auc, &lines, ftrl::print_field_importance);
    loss.pop_back();
    check(lines == -1 && short_auc.empty() && ftrl::print_field_importance(stdout, 3, 8, loss, nullptr) == -1,
          "a loss or AUC vector of the wrong length prints no field line");
    const std::string none = printed(argv[3], 2, 0, {0.0, 0.0, 0.0}, nullptr, &lines, ftrl::print_field_importance);
    check(lines == 2 && none == "field importance: 0 rows, loss 0.000000\n"
                                "field 0: without it loss 0.000000 (delta +0.000000)\n"
                                "field 1: without it loss 0.000000 (delta +0.000000)\n",
          "the fields' lines of an empty file");
  }
  if (argc == 5) {
    // the engine library's numbering -- ffm_engine_pair_count / _pair_index, which are the kernel header's pair_base
    // and pair_variants -- against this file's copy, every pair of 1 .. 64 fields in both orders
    void *lib = dlopen(argv[4], RTLD_NOW | RTLD_LOCAL);
    using CountFn = int32_t (*)(int32_t);
    using IndexFn = int32_t (*)(int32_t, int32_t, int32_t);
    CountFn count = lib ? reinterpret_cast<CountFn>(dlsym(lib, "ffm_engine_pair_count")) : nullptr;
    IndexFn index = lib ? reinterpret_cast<IndexFn>(dlsym(lib, "ffm_engine_pair_index")) : nullptr;
    bool ok = count && index;
    for (int F = 1; ok && F <= 64; F++) {
      ok = count(F) == ftrl::pair_count(F);
      for (int f = 0; ok && f < F; f++)
        for (int g = f; ok && g < F; g++) ok = index(F, f, g) == ftrl::pair_index(F, f, g) && index(F, g, f) == ftrl::pair_index(F, f, g);
    }
    check(ok, "the engine library numbers the pairs as host/importance.h does");
  }
  std::printf("%d ok, %d failed\n", n_ok, n_fail);
  return n_fail == 0 ? 0 : 1;
}
