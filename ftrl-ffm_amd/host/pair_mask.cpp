#include "pair_mask.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <numeric>
#include <sstream>
#include <stdexcept>

namespace ftrl {

namespace {
int count_of(int n_fields) { return n_fields * (n_fields + 1) / 2; }
int index_of(int n_fields, int f, int g) { return f * n_fields - f * (f - 1) / 2 + (g - f); }
void check_fields(int n_fields) {
  if (n_fields < 1 || n_fields > 64)
    throw std::invalid_argument("a pair mask is for 1 .. 64 fields, got n_fields = " + std::to_string(n_fields));
}
}  // namespace

std::vector<int> rank_pairs(int n_fields, const std::vector<double> &loss) {
  check_fields(n_fields);
  const int V = count_of(n_fields);
  if (loss.size() != static_cast<size_t>(V) + 1)
    throw std::invalid_argument("pair mask: " + std::to_string(V + 1) + " loss sums expected, got " + std::to_string(loss.size()));
  std::vector<double> delta(static_cast<size_t>(V));
  size_t v = 0;
  for (int f = 0; f < n_fields; f++)
    for (int g = f; g < n_fields; g++, v++) {  // (v == index_of(n_fields, f, g): the pairs in index order)
      delta[v] = loss[v] - loss[static_cast<size_t>(V)];
      if (!std::isfinite(delta[v]))
        throw std::runtime_error("pair mask: loss without pair " + std::to_string(f) + " " + std::to_string(g) + " is not finite");
    }
  std::vector<int> order(static_cast<size_t>(V));
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return delta[a] > delta[b]; });
  return order;
}

PairList select_pairs(int n_fields, const std::vector<double> &loss, int n_keep, double *smallest_kept) {
  check_fields(n_fields);
  const int V = count_of(n_fields);
  if (loss.size() != static_cast<size_t>(V) + 1)
    throw std::invalid_argument("pair mask: " + std::to_string(V + 1) + " loss sums expected, got " + std::to_string(loss.size()));
  if (n_keep < 0 || n_keep > V)
    throw std::invalid_argument("--pair_keep must lie in [0, " + std::to_string(V) + "], got " + std::to_string(n_keep));
  std::vector<int> order = rank_pairs(n_fields, loss);
  if (smallest_kept) {
    const size_t last = n_keep > 0 ? static_cast<size_t>(order[static_cast<size_t>(n_keep) - 1]) : 0;
    *smallest_kept = n_keep > 0 ? loss[last] - loss[static_cast<size_t>(V)] : 0.0;
  }
  order.resize(static_cast<size_t>(n_keep));
  std::sort(order.begin(), order.end());
  PairList all;
  for (int f = 0; f < n_fields; f++)
    for (int g = f; g < n_fields; g++) all.emplace_back(f, g);
  PairList kept;
  for (int v : order) kept.push_back(all[static_cast<size_t>(v)]);
  return kept;
}

std::vector<uint16_t> pair_curve_levels(int n_fields, const std::vector<int> &order) {
  check_fields(n_fields);
  const int V = count_of(n_fields);
  std::vector<int> rank(static_cast<size_t>(V), -1);
  if (order.size() != static_cast<size_t>(V)) throw std::invalid_argument("pair curve: the order must list all " + std::to_string(V) + " pairs");
  for (int at = 0; at < V; at++) {
    const int v = order[static_cast<size_t>(at)];
    if (v < 0 || v >= V || rank[static_cast<size_t>(v)] >= 0) throw std::invalid_argument("pair curve: the order is no permutation of the pairs");
    rank[static_cast<size_t>(v)] = at;
  }
  std::vector<uint16_t> level(static_cast<size_t>(n_fields) * n_fields);
  for (int f = 0; f < n_fields; f++)
    for (int g = f; g < n_fields; g++) {
      const uint16_t at = static_cast<uint16_t>(rank[static_cast<size_t>(index_of(n_fields, f, g))]);  // (V <= 2080)
      level[static_cast<size_t>(f) * n_fields + g] = level[static_cast<size_t>(g) * n_fields + f] = at;
    }
  return level;
}

int pick_by_budget(const std::vector<int> &keep, const std::vector<double> &curve_loss, unsigned long long rows, double budget) {
  if (curve_loss.size() != keep.size() + 1) throw std::invalid_argument("pair curve: one loss sum per listed number of pairs and the rows' own");
  const double n = rows ? static_cast<double>(rows) : 1.0;
  for (size_t i = 0; i < keep.size(); i++) {
    const double delta = (curve_loss[i] - curve_loss.back()) / n;
    if (std::isfinite(delta) && delta <= budget) return static_cast<int>(i);
  }
  return -1;
}

std::vector<uint64_t> pair_mask_words(int n_fields, const PairList &pairs) {
  check_fields(n_fields);
  std::vector<uint64_t> keep(static_cast<size_t>(n_fields), 0);
  for (const auto &[f, g] : pairs) {
    if (f < 0 || g < 0 || f >= n_fields || g >= n_fields)
      throw std::invalid_argument("pair (" + std::to_string(f) + ", " + std::to_string(g) + ") names a field outside [0, n_fields)");
    keep[static_cast<size_t>(f)] |= uint64_t{1} << g;
    keep[static_cast<size_t>(g)] |= uint64_t{1} << f;
  }
  return keep;
}

void write_pair_mask(const std::string &path, int n_fields, const PairList &pairs) {
  std::FILE *f = std::fopen(path.c_str(), "w");
  if (!f) throw std::runtime_error("--pair_mask_out: cannot write " + path);
  bool ok = std::fprintf(f, "ffm-pair-mask 1 %d %zu\n", n_fields, pairs.size()) > 0;
  for (const auto &p : pairs) ok = ok && std::fprintf(f, "%d %d\n", p.first, p.second) > 0;
  ok = std::fclose(f) == 0 && ok;
  if (!ok) throw std::runtime_error("--pair_mask_out: writing " + path + " failed");
}

PairList read_pair_mask(const std::string &path, int n_fields) {
  check_fields(n_fields);
  std::ifstream in(path);
  if (!in.good()) throw std::invalid_argument(path + ": cannot be opened");
  auto at = [&](size_t line, const std::string &msg) { return std::invalid_argument(path + ":" + std::to_string(line) + ": " + msg); };
  // a line's tokens, all of them: trailing text is an error, not ignored
  auto tokens = [](const std::string &text) {
    std::istringstream ss(text);
    std::vector<std::string> out;
    for (std::string t; ss >> t;) out.push_back(t);
    return out;
  };
  auto number = [&](const std::string &t, size_t line) {
    if (t.empty() || t.size() > 9 || !std::all_of(t.begin(), t.end(), [](char c) { return c >= '0' && c <= '9'; }))
      throw at(line, "not a number: `" + t + "`");
    return std::stoi(t);
  };
  std::string text;
  if (!std::getline(in, text)) throw at(1, "empty file: `ffm-pair-mask 1 <n_fields> <n_kept>` expected");
  const std::vector<std::string> head = tokens(text);
  if (head.empty() || head[0] != "ffm-pair-mask") throw at(1, "not a pair mask file: the first line must start with ffm-pair-mask");
  if (head.size() != 4) throw at(1, "`ffm-pair-mask 1 <n_fields> <n_kept>` expected");
  if (number(head[1], 1) != 1) throw at(1, "version " + head[1] + " is not supported (1 is)");
  const int file_fields = number(head[2], 1), n_kept = number(head[3], 1);
  if (file_fields != n_fields)
    throw at(1, "the mask is for " + std::to_string(file_fields) + " fields, this run has n_fields = " + std::to_string(n_fields));
  const int V = count_of(n_fields);
  if (n_kept > V) throw at(1, std::to_string(n_kept) + " pairs kept, " + std::to_string(n_fields) + " fields have " + std::to_string(V));
  PairList pairs;
  int last = -1;
  size_t line = 1;
  while (std::getline(in, text)) {
    line++;
    const std::vector<std::string> t = tokens(text);
    if (t.empty()) continue;
    if (t.size() != 2) throw at(line, "`f g` expected, got `" + text + "`");
    const int f = number(t[0], line), g = number(t[1], line);
    if (f >= n_fields || g >= n_fields) throw at(line, "pair " + t[0] + " " + t[1] + " names a field outside [0, " + std::to_string(n_fields) + ")");
    if (f > g) throw at(line, "pair " + t[0] + " " + t[1] + ": f <= g expected");
    const int v = index_of(n_fields, f, g);
    if (v == last) throw at(line, "pair " + t[0] + " " + t[1] + " is listed twice");
    if (v < last) throw at(line, "pair " + t[0] + " " + t[1] + " is out of order: the pair index must ascend");
    if (static_cast<int>(pairs.size()) == n_kept) throw at(line, "more pairs than the " + std::to_string(n_kept) + " the header counts");
    last = v;
    pairs.emplace_back(f, g);
  }
  if (static_cast<int>(pairs.size()) != n_kept)
    throw at(line, std::to_string(pairs.size()) + " pairs, the header counts " + std::to_string(n_kept));
  return pairs;
}

}  // namespace ftrl
