// Stand-alone program over ftrl-ffm_amd/host/sample_weights.cpp alone (no engine, no device): the
// weight-file reader, the row counter and the flag checks of the trainer CLI.  Built by
// tests/test_sample_weights_host.py with g++, plain and with -fsanitize=address,undefined.
//   usage: sample_weights_file <scratch directory>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <stdexcept>
#include <string>

#include "../ftrl-ffm_amd/host/sample_weights.h"

static int n_ok = 0, n_failed = 0;
static void expect(bool cond, const std::string &what) {
  std::printf("%s %s\n", cond ? "ok  " : "FAIL", what.c_str());
  (cond ? n_ok : n_failed)++;
}
static void write(const std::string &path, const std::string &text) {
  std::ofstream f(path, std::ios::binary);
  f << text;
}
// the message of the exception `fn` throws ("" when it throws nothing)
template <typename Fn>
static std::string thrown(Fn fn) {
  try {
    fn();
  } catch (const std::exception &e) {
    return e.what();
  }
  return "";
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  const std::string dir = argv[1], w = dir + "/w.txt", d = dir + "/d.ffm";

  // ---- the reader
  write(w, "1\n0.25\n+3.5\n1e-3\n64 \r\n  0\n2.5");  // spellings, blanks around, CRLF, no newline at the end
  const std::vector<float> got = ftrl::read_weight_file(w);
  const float want[7] = {1.0f, 0.25f, 3.5f, 1e-3f, 64.0f, 0.0f, 2.5f};
  bool same = got.size() == 7;
  for (size_t i = 0; same && i < 7; i++) same = got[i] == want[i];
  expect(same, "read: seven spellings");
  write(w, "");
  expect(ftrl::read_weight_file(w).empty(), "read: empty file");
  const struct { const char *text, *at, *why; } bad[] = {
      {"1\nabc\n1\n", ":2:", "cannot parse"}, {"1\n1\n1.0x\n", ":3:", "cannot parse"}, {"\n1\n", ":1:", "cannot parse"},
      {"1\n-0.5\n", ":2:", "negative"},       {"inf\n", ":1:", "not finite"},          {"1\nnan\n", ":2:", "not finite"},
      {"1\n1e99\n", ":2:", "not finite"},     {"1 2\n", ":1:", "cannot parse"},        {"-inf\n", ":1:", "not finite"},
      {"1\n-\n", ":2:", "cannot parse"},
  };
  for (const auto &b : bad) {
    write(w, b.text);
    const std::string msg = thrown([&] { ftrl::read_weight_file(w); });
    expect(msg.find(w + b.at) != std::string::npos && msg.find(b.why) != std::string::npos,
           std::string("reject ") + b.why + " at" + b.at + " -> " + msg);
  }
  expect(!thrown([&] { ftrl::read_weight_file(dir + "/none.txt"); }).empty(), "reject a missing file");

  // ---- rows as the parsers count them: lines that hold anything but blanks
  write(d, "1 0:1:1\n\n0 0:2:1\r\n   \n1 0:3:1");
  expect(ftrl::count_data_rows(d) == 3, "count: blank lines, CRLF, no newline at the end");
  write(d, "");
  expect(ftrl::count_data_rows(d) == 0, "count: empty file");

  // ---- the flags together
  config_options opt;
  opt.train_path = d;
  write(d, "1 0:1:1\n0 0:2:1\n1 0:3:1\n");
  expect(!ftrl::load_sample_weights(opt).on, "no flag: off, nothing read");
  opt.weights_given = true;
  opt.pos_weight = 0.5f;
  opt.neg_weight = 2.5f;
  ftrl::SampleWeights sw = ftrl::load_sample_weights(opt);
  expect(sw.on && sw.file.empty() && sw.of(0, 1) == 0.5f && sw.of(7, 0) == 2.5f, "class weights alone");
  write(w, "2\n4\n0\n");
  opt.weight_path = w;
  sw = ftrl::load_sample_weights(opt);
  expect(sw.of(0, 1) == 1.0f && sw.of(1, 0) == 10.0f && sw.of(2, 1) == 0.0f, "file weight x class weight");
  CsrBlock blk;
  blk.push(Sample{{{0, 1, 1.0f}}, 1});
  blk.push(Sample{{{0, 2, 1.0f}}, 0});
  const int idx[2] = {2, 1};
  double sum = sw.fill(blk, idx, 0);
  expect(blk.weight.size() == 2 && blk.weight[0] == 0.0f && blk.weight[1] == 10.0f && sum == 10.0, "fill by row index");
  sum = sw.fill(blk, nullptr, 0);
  expect(blk.weight[0] == 1.0f && blk.weight[1] == 10.0f && sum == 11.0, "fill in file order");
  blk.clear();
  expect(blk.weight.empty(), "clear() drops the weights");
  write(w, "2\n4\n");
  std::string msg = thrown([&] { ftrl::load_sample_weights(opt); });
  expect(msg.find(w + ":3:") != std::string::npos && msg.find("2 weights") != std::string::npos && msg.find("3 rows") != std::string::npos,
         "reject a short file -> " + msg);
  write(w, "2\n4\n1\n1\n");
  msg = thrown([&] { ftrl::load_sample_weights(opt); });
  expect(msg.find(w + ":4:") != std::string::npos, "reject a long file -> " + msg);
  opt.weight_path.clear();
  opt.neg_weight = -1.0f;
  expect(!thrown([&] { ftrl::load_sample_weights(opt); }).empty(), "reject a negative class weight");
  opt.neg_weight = NAN;
  expect(!thrown([&] { ftrl::load_sample_weights(opt); }).empty(), "reject a NaN class weight");
  opt.neg_weight = INFINITY;
  expect(!thrown([&] { ftrl::load_sample_weights(opt); }).empty(), "reject an infinite class weight");

  std::printf("%d ok, %d failed\n", n_ok, n_failed);
  return n_failed ? 1 : 0;
}
