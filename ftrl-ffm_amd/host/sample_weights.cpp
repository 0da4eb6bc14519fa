#include "sample_weights.h"

#include <algorithm>
#include <charconv>
#include <cmath>
#include <cstring>
#include <fstream>
#include <stdexcept>

namespace ftrl {

double SampleWeights::fill(CsrBlock &blk, const int *idx, size_t first) const {
  const size_t n = static_cast<size_t>(blk.n_rows());
  blk.weight.resize(n);
  double sum = 0.0;
  for (size_t j = 0; j < n; j++) {
    const float w = of(idx ? static_cast<size_t>(idx[j]) : first + j, blk.label[j]);
    blk.weight[j] = w;
    sum += static_cast<double>(w);
  }
  return sum;
}

size_t count_data_rows(const std::string &path) {
  std::ifstream in(path, std::ios::binary);
  if (!in.good()) throw std::runtime_error("cannot open " + path);
  std::vector<char> buf(1 << 20);
  size_t rows = 0;
  bool content = false;  // the current line holds something other than blanks
  for (;;) {
    in.read(buf.data(), static_cast<std::streamsize>(buf.size()));
    const std::streamsize got = in.gcount();
    if (got <= 0) break;
    for (std::streamsize i = 0; i < got; i++) {
      const char c = buf[static_cast<size_t>(i)];
      if (c == '\n') { rows += content ? 1 : 0; content = false; }
      else if (c != ' ' && c != '\r') content = true;
    }
  }
  return rows + (content ? 1 : 0);
}

std::vector<float> read_weight_file(const std::string &path) {
  std::ifstream in(path);
  if (!in.good()) throw std::runtime_error("cannot open " + path);
  std::vector<float> out;
  std::string line;
  size_t no = 0;
  while (std::getline(in, line)) {
    no++;
    const auto bad = [&](const char *what) {
      return std::runtime_error(path + ":" + std::to_string(no) + ": " + what + ": `" + line + "`");
    };
    const char *b = line.data(), *e = b + line.size();
    while (e > b && (e[-1] == '\r' || e[-1] == ' ' || e[-1] == '\t')) e--;
    while (b < e && (*b == ' ' || *b == '\t')) b++;
    if (b < e && *b == '+') b++;
    float v = 0.0f;
    const auto r = std::from_chars(b, e, v);
    if (r.ec == std::errc::result_out_of_range) throw bad("weight is not finite");
    if (b == e || r.ec != std::errc() || r.ptr != e) throw bad("cannot parse weight");
    if (std::isnan(v) || std::isinf(v)) throw bad("weight is not finite");
    if (v < 0.0f) throw bad("weight is negative");
    out.push_back(v);
  }
  return out;
}

SampleWeights load_sample_weights(const config_options &opt) {
  SampleWeights w;
  w.on = opt.weights_given;
  if (!w.on) return w;
  for (const float c : {opt.pos_weight, opt.neg_weight})
    if (!(c >= 0.0f) || std::isinf(c)) throw std::invalid_argument("--pos_weight / --neg_weight take finite values >= 0");
  w.pos = opt.pos_weight;
  w.neg = opt.neg_weight;
  if (!opt.weight_path.empty()) {
    w.file = read_weight_file(opt.weight_path);
    const size_t rows = opt.train_path.empty() ? 0 : count_data_rows(opt.train_path);
    if (w.file.size() != rows)
      throw std::runtime_error(opt.weight_path + ":" + std::to_string(std::min(w.file.size(), rows) + 1) + ": holds " +
                               std::to_string(w.file.size()) + " weights, " + opt.train_path + " has " +
                               std::to_string(rows) + " rows");
  }
  return w;
}

}  // namespace ftrl
