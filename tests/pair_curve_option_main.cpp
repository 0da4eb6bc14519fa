// Stand-alone check of --pair_curve and --pair_loss_budget in host/cmd_option.cpp, and of what host/pair_mask.cpp and
// host/importance.cpp add for them (no GPU, no engine library): every accepted spelling, every refusal -- all made
// while the options are parsed, before a device is opened --, the old --pair_keep / --pair_mask_out refusals with their
// old messages, the auto list, the ranking, the level table, the budget's pick and the printed lines.  Built and run
// by tests/test_pair_curve_host.py, once plainly and once under -fsanitize=address,undefined.
//   usage: pair_curve_option <libffm file> <scratch file>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../ftrl-ffm_amd/host/cmd_option.h"
#include "../ftrl-ffm_amd/host/importance.h"
#include "../ftrl-ffm_amd/host/pair_mask.h"

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

static std::vector<int> auto_list(int V) {  // round(i V / 63), i = 0 .. 63, deduplicated: the issue's sentence in doubles
  std::vector<int> out;
  for (int i = 0; i < 64; i++) {
    const int n = static_cast<int>(static_cast<double>(i) * V / 63.0 + 0.5);
    if (out.empty() || out.back() != n) out.push_back(n);
  }
  return out;
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  const std::string ffm = argv[1];
  using V = std::vector<std::string>;
  using L = std::vector<int>;
  const V base = {"--model_type", "FFM", "--n_fields", "8", "--train_data", ffm, "--eval_data", ffm};  // 36 pairs
  auto with = [&](V more) {
    V all = base;
    all.insert(all.end(), more.begin(), more.end());
    return all;
  };
  const V imp = {"--pair_importance", "true"};
  auto curve = [&](V more) {
    V all = with(imp);
    all.insert(all.end(), more.begin(), more.end());
    return all;
  };

  // ---- accepted
  {
    const config_options o = parse(base);
    check(o.pair_curve.empty() && o.pair_curve_keep.empty() && !o.pair_loss_budget_set, "the default: no curve, no budget");
  }
  check(parse(curve({"--pair_curve", "0,5,36"})).pair_curve_keep == L({0, 5, 36}), "--pair_curve 0,5,36");
  check(parse(curve({"--pair_curve", "7"})).pair_curve_keep == L({7}), "--pair_curve 7: one N");
  check(parse(curve({"--pair_curve", "36,0,5,5,0"})).pair_curve_keep == L({0, 5, 36}), "any order, duplicates: ascending, once each");
  check(parse(curve({"--pair_curve", "auto"})).pair_curve_keep == auto_list(36), "--pair_curve auto at 8 fields");
  check(parse({"--model_type", "FFM", "--pair_curve", "auto", "--pair_importance", "true", "--train_data", ffm, "--eval_data", ffm, "--n_fields", "39"})
                .pair_curve_keep == auto_list(780) &&
            parse({"--model_type", "FFM", "--pair_curve", "780", "--pair_importance", "true", "--train_data", ffm, "--eval_data", ffm, "--n_fields",
                   "39"}).pair_curve_keep == L({780}),
        "--n_fields after --pair_curve: the list is made once both are known");
  {
    bool ok = true;
    for (int F : {6, 39, 64}) {
      const int Vn = F * (F + 1) / 2;
      const L a = parse({"--model_type", "FFM", "--n_fields", std::to_string(F), "--train_data", ffm, "--eval_data", ffm, "--pair_importance",
                         "true", "--pair_curve", "auto"}).pair_curve_keep;
      ok = ok && a == auto_list(Vn) && a.front() == 0 && a.back() == Vn && a.size() <= 64;
      if (F == 6) ok = ok && a.size() == 22;   // V = 21 < 64: every N once
      if (F != 6) ok = ok && a.size() == 64;
    }
    check(ok, "auto for V = 21, 780 and 2080");
    std::string list;
    for (int i = 0; i < 64; i++) list += (i ? "," : "") + std::to_string(i % 37);
    check(parse(curve({"--pair_curve", list})).pair_curve_keep.size() == 37, "64 entries are accepted");
  }
  {
    const config_options o = parse(curve({"--pair_curve", "0,5,36", "--pair_loss_budget", "0.001", "--pair_mask_out", "m.txt"}));
    check(o.pair_loss_budget_set && o.pair_loss_budget == 0.001 && o.pair_mask_out == "m.txt" && o.pair_keep == -1, "--pair_loss_budget 0.001");
    check(parse(curve({"--pair_curve", "auto", "--pair_loss_budget", "-1e-3", "--pair_mask_out", "m.txt"})).pair_loss_budget == -1e-3 &&
              parse(curve({"--pair_curve", "auto", "--pair_loss_budget", "0", "--pair_mask_out", "m.txt"})).pair_loss_budget_set,
          "a negative and a zero budget");
    check(refusal(curve({"--pair_curve", "0,5", "--pair_keep", "5", "--pair_mask_out", "m.txt"})).empty(), "--pair_curve beside --pair_keep N --pair_mask_out");
    check(refusal(curve({"--pair_curve", "0,5", "--metrics", "auc", "--field_importance", "true"})).empty(), "with --metrics auc and --field_importance true");
    check(refusal({"--model_type", "FFM", "--n_fields", "8", "--eval_data", ffm, "--resume_from", "ck", "--n_epochs", "0", "--predict_data", ffm,
                   "--predict_out", "p.txt", "--serve_weights", "f16", "--pair_importance", "true", "--pair_curve", "auto"}).empty(),
          "--resume_from ck --n_epochs 0 --serve_weights f16");
  }

  // ---- refused
  {
    const std::string msg = refusal(with({"--pair_curve", "0,5"}));
    check(has(msg, "--pair_curve 0,5 ") && has(msg, "it needs --pair_importance true"), "refused: --pair_curve without --pair_importance true");
    check(has(refusal(with({"--pair_curve", "auto", "--pair_importance", "false"})), "it needs --pair_importance true"),
          "refused: --pair_curve auto with --pair_importance false");
  }
  {
    bool ok = true;
    for (const char *bad : {"", ",", "1,", ",1", "1,,2", "a", "1,b", "-1", "1.5", "1 2", "0x10", "12345", "autos", "Auto", "+3"}) {
      const std::string msg = refusal(curve({"--pair_curve", bad}));
      ok = ok && has(msg, "--pair_curve takes auto or 1 to 64 comma-separated numbers of pairs");
      if (!ok) std::printf("     (`%s` gave `%s`)\n", bad, msg.c_str());
    }
    check(ok, "refused: malformed lists");
    std::string list;
    for (int i = 0; i < 65; i++) list += (i ? "," : "") + std::to_string(i % 37);
    check(has(refusal(curve({"--pair_curve", list})), "at most 64 numbers of pairs"), "refused: 65 entries");
    const std::string msg = refusal(curve({"--pair_curve", "0,37"}));
    check(has(msg, "37 is more than the 36 pairs of --n_fields 8"), "refused: an N above V");
  }
  {
    const std::string both = refusal(curve({"--pair_curve", "0,5", "--pair_loss_budget", "0.1", "--pair_keep", "5", "--pair_mask_out", "m.txt"}));
    check(has(both, "--pair_loss_budget") && has(both, "--pair_keep") && has(both, "not allowed together"), "refused: --pair_loss_budget with --pair_keep");
    check(has(refusal(with({"--pair_importance", "true", "--pair_loss_budget", "0.1", "--pair_mask_out", "m.txt"})), "it needs --pair_curve"),
          "refused: --pair_loss_budget without --pair_curve");
    check(has(refusal(curve({"--pair_curve", "0,5", "--pair_loss_budget", "0.1"})), "it needs --pair_mask_out"),
          "refused: --pair_loss_budget without --pair_mask_out");
    bool ok = true;
    for (const char *bad : {"", "x", "0.1x", "nan", "inf", "1e999"})
      ok = ok && has(refusal(curve({"--pair_curve", "0,5", "--pair_mask_out", "m.txt", "--pair_loss_budget", bad})), "--pair_loss_budget takes a finite per-row loss delta");
    check(ok, "refused: a budget that is no finite number");
  }
  // ---- the old refusals, with their old messages
  check(refusal(with({"--pair_importance", "true", "--pair_mask_out", "m.txt"})) ==
            "--pair_mask_out writes the pairs --pair_keep N selects: it needs --pair_keep",
        "old: --pair_mask_out without --pair_keep");
  check(refusal(curve({"--pair_curve", "0,5", "--pair_mask_out", "m.txt"})) == "--pair_mask_out writes the pairs --pair_keep N selects: it needs --pair_keep",
        "old: --pair_mask_out without --pair_keep, beside a curve without a budget");
  check(refusal(with({"--pair_importance", "true", "--pair_keep", "5"})) == "--pair_keep selects the pairs --pair_mask_out FILE writes: it needs --pair_mask_out",
        "old: --pair_keep without --pair_mask_out");
  check(refusal(with({"--pair_keep", "5", "--pair_mask_out", "m.txt"})) ==
            "--pair_keep 5 ranks the pairs by the pair importance pass: it needs --pair_importance true",
        "old: --pair_keep without --pair_importance true");
  check(refusal(with({"--pair_importance", "true", "--pair_keep", "37", "--pair_mask_out", "m.txt"})) ==
            "--pair_keep 37 is more than the 36 pairs of --n_fields 8",
        "old: --pair_keep above V");
  check(refusal(with({"--pair_importance", "true", "--pair_keep", "x", "--pair_mask_out", "m.txt"})) ==
            "--pair_keep takes a number of pairs in [0, 2080], got `x`",
        "old: --pair_keep that is no number");
  check(refusal(with({"--pair_importance", "true", "--pair_keep", "5", "--pair_mask_out", "m.txt"})).empty(), "old: --pair_keep 5 --pair_mask_out parses");
  check(std::string(cmd_help).find("--pair_curve <LIST|auto>") != std::string::npos && std::string(cmd_help).find("--pair_loss_budget <T>") != std::string::npos,
        "the help names the flags");

  // ---- host/pair_mask.cpp: the ranking, the level table, the budget's pick
  {
    // 3 fields, 6 pairs; deltas 0, +1, 0, -0.5, +1, +0.25: best first is 1, 4 (tie: the lower index), 5, 0, 2 (tie), 3
    const std::vector<double> loss = {4.0, 5.0, 4.0, 3.5, 5.0, 4.25, 4.0};
    const std::vector<int> order = ftrl::rank_pairs(3, loss);
    check(order == L({1, 4, 5, 0, 2, 3}), "rank_pairs: largest delta first, ties to the lower index");
    bool ok = true;
    for (int n = 0; n <= 6; n++) {
      ftrl::PairList want;
      std::vector<int> first(order.begin(), order.begin() + n);
      for (int f = 0; f < 3; f++)
        for (int g = f; g < 3; g++)
          for (int v : first)
            if (v == ftrl::pair_index(3, f, g)) want.emplace_back(f, g);
      ok = ok && ftrl::select_pairs(3, loss, n) == want;
    }
    double smallest = -1.0;
    ftrl::select_pairs(3, loss, 3, &smallest);
    check(ok && smallest == 0.25, "select_pairs keeps the ranking's first N, and the smallest kept delta is what it was");
    const std::vector<uint16_t> level = ftrl::pair_curve_levels(3, order);
    // pairs in index order: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2) at ranks 3 0 4 5 1 2
    check(level == std::vector<uint16_t>({3, 0, 4, 0, 5, 1, 4, 1, 2}), "pair_curve_levels: the rank, symmetric, row-major");
    ok = true;
    for (int n = 0; n <= 6; n++) {  // cut n keeps exactly select_pairs(.., n)
      ftrl::PairList below;
      for (int f = 0; f < 3; f++)
        for (int g = f; g < 3; g++)
          if (level[static_cast<size_t>(f * 3 + g)] < n) below.emplace_back(f, g);
      ok = ok && below == ftrl::select_pairs(3, loss, n);
    }
    check(ok, "level < N is select_pairs(N), for every N");
    bool threw = false;
    try { ftrl::pair_curve_levels(3, {0, 1, 2, 3, 4, 4}); } catch (const std::invalid_argument &) { threw = true; }
    bool threw_short = false;
    try { ftrl::pair_curve_levels(3, {0, 1, 2}); } catch (const std::invalid_argument &) { threw_short = true; }
    check(threw && threw_short, "pair_curve_levels refuses what is no permutation");
  }
  {
    const L keep = {0, 2, 4, 6};
    const std::vector<double> loss = {16.0, 9.0, 8.5, 8.0, 8.0};  // 8 rows: deltas 1, 0.125, 0.0625, 0
    check(ftrl::pick_by_budget(keep, loss, 8, 0.125) == 1 && ftrl::pick_by_budget(keep, loss, 8, 0.1) == 2 && ftrl::pick_by_budget(keep, loss, 8, 0.0) == 3 &&
              ftrl::pick_by_budget(keep, loss, 8, 5.0) == 0,
          "pick_by_budget: the smallest listed N whose delta is <= T");
    check(ftrl::pick_by_budget(keep, loss, 8, -0.001) == -1 && ftrl::pick_by_budget({0}, {16.0, 8.0}, 8, 0.5) == -1, "pick_by_budget: none meets it");
    const double nan = std::stod("nan");
    check(ftrl::pick_by_budget({0, 6}, {nan, 8.0, 8.0}, 8, 0.5) == 1, "pick_by_budget: a delta that is not finite meets no budget");
  }
  // ---- host/importance.cpp: the lines
  {
    const L keep = {0, 2, 6};
    const std::vector<double> loss = {5.0, 3.5, 4.0, 4.0};
    std::FILE *f = std::fopen(argv[2], "w");
    const int lines = f ? ftrl::print_pair_curve(f, 3, 8, keep, loss, nullptr) : -2;
    if (f) std::fclose(f);
    std::stringstream s;
    s << std::ifstream(argv[2]).rdbuf();
    check(lines == 3 && s.str() == "pair curve: 8 rows, loss 0.500000\n"
                                   "keep 0 of 6 pairs: loss 0.625000 (delta +0.125000)\n"
                                   "keep 2 of 6 pairs: loss 0.437500 (delta -0.062500)\n"
                                   "keep 6 of 6 pairs: loss 0.500000 (delta +0.000000)\n",
          "the lines without AUC");
    std::vector<ffm_metrics> auc(4);
    for (auto &m : auc) m.auc = 0.75;
    auc[0].auc = 0.5;
    f = std::fopen(argv[2], "w");
    const int with_auc = f ? ftrl::print_pair_curve(f, 3, 8, keep, loss, &auc) : -2;
    if (f) std::fclose(f);
    std::stringstream t;
    t << std::ifstream(argv[2]).rdbuf();
    check(with_auc == 3 && t.str() == "pair curve: 8 rows, loss 0.500000, auc 0.750000\n"
                                      "keep 0 of 6 pairs: loss 0.625000 (delta +0.125000), auc 0.500000 (delta -0.250000)\n"
                                      "keep 2 of 6 pairs: loss 0.437500 (delta -0.062500), auc 0.750000 (delta +0.000000)\n"
                                      "keep 6 of 6 pairs: loss 0.500000 (delta +0.000000), auc 0.750000 (delta +0.000000)\n",
          "the lines with AUC");
    auc.pop_back();
    check(ftrl::print_pair_curve(stdout, 3, 8, keep, loss, &auc) == -1 && ftrl::print_pair_curve(stdout, 3, 8, {0, 2}, loss, nullptr) == -1,
          "a loss or AUC vector of the wrong length prints nothing");
  }
  std::printf("%d ok, %d failed\n", n_ok, n_fail);
  return n_fail == 0 ? 0 : 1;
}
