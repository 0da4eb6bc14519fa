// metrics_host_main.cpp -- stand-alone check of csrc/metrics_host.h (histogram -> AUC in integers):
// built by tests/test_metrics_host.py with g++ alone, plainly and with -fsanitize=address,undefined,
// and run directly.  Every case is compared with a pair-by-pair count over the bins (quadratic, in a
// 128-bit accumulator of its own) and with closed forms.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../ftrl-ffm_amd/csrc/metrics_host.h"

typedef unsigned __int128 u128;

static int n_checks = 0, n_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    n_checks++;                                                            \
    if (!(cond)) {                                                         \
      n_failed++;                                                          \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
    }                                                                      \
  } while (0)

static bool same_double(double a, double b) { return (std::isnan(a) && std::isnan(b)) || a == b; }

// U2 and T by looking at every pair of bins
static void brute(const std::vector<uint64_t> &pos, const std::vector<uint64_t> &neg, ffm_metrics *want) {
  u128 u2 = 0, ties = 0, P = 0, N = 0;
  int64_t mixed = 0;
  const size_t n = pos.size();
  for (size_t b = 0; b < n; b++) {
    P += pos[b];
    N += neg[b];
    if (pos[b] && neg[b]) mixed++;
    ties += static_cast<u128>(pos[b]) * neg[b];
    for (size_t c = 0; c < b; c++) u2 += 2 * (static_cast<u128>(pos[b]) * neg[c]);
  }
  u2 += ties;
  want->n_pos = static_cast<int64_t>(P);
  want->n_neg = static_cast<int64_t>(N);
  want->n_mixed_bins = mixed;
  if (P == 0 || N == 0) {
    want->auc = want->auc_slack = NAN;
  } else {
    want->auc = static_cast<double>(u2) / static_cast<double>(2 * P * N);
    want->auc_slack = static_cast<double>(ties) / static_cast<double>(2 * P * N);
  }
}

static void compare(const std::vector<uint64_t> &pos, const std::vector<uint64_t> &neg, int64_t n_nan) {
  ffm_metrics got{}, want{};
  const int rc = ffm_metrics_host::from_histogram(pos.data(), neg.data(), static_cast<int64_t>(pos.size()), n_nan, &got);
  brute(pos, neg, &want);
  CHECK(rc == FFM_OK);
  CHECK(got.n_pos == want.n_pos && got.n_neg == want.n_neg && got.n_mixed_bins == want.n_mixed_bins);
  CHECK(got.n_nan == n_nan);
  CHECK(same_double(got.auc, want.auc));
  CHECK(same_double(got.auc_slack, want.auc_slack));
}

int main() {
  std::mt19937_64 rng(20);
  // random histograms of every small size, dense and sparse, small and 40-bit counts
  for (int n_bins : {1, 2, 3, 7, 64, 257}) {
    for (int rep = 0; rep < 8; rep++) {
      std::vector<uint64_t> pos(n_bins), neg(n_bins);
      const bool sparse = rep & 1, large = rep & 2;
      for (int b = 0; b < n_bins; b++) {
        const uint64_t cap = large ? (1ull << 40) : 9;
        pos[b] = sparse && rng() % 3 ? 0 : rng() % cap;
        neg[b] = sparse && rng() % 3 ? 0 : rng() % cap;
      }
      compare(pos, neg, rep);
    }
  }
  // all ties: one bin holds everything -> auc 1/2, slack 1/2
  {
    ffm_metrics m{};
    const uint64_t p = 5, n = 11;
    CHECK(ffm_metrics_host::from_histogram(&p, &n, 1, 0, &m) == FFM_OK);
    CHECK(m.auc == 0.5 && m.auc_slack == 0.5 && m.n_mixed_bins == 1 && m.n_pos == 5 && m.n_neg == 11);
  }
  // perfectly separated, both ways round
  {
    ffm_metrics m{};
    const uint64_t lo[2] = {7, 0}, hi[2] = {0, 3};
    CHECK(ffm_metrics_host::from_histogram(hi, lo, 2, 0, &m) == FFM_OK);
    CHECK(m.auc == 1.0 && m.auc_slack == 0.0 && m.n_mixed_bins == 0);
    CHECK(ffm_metrics_host::from_histogram(lo, hi, 2, 0, &m) == FFM_OK);
    CHECK(m.auc == 0.0 && m.auc_slack == 0.0);
  }
  // counts of 2^33 in two bins: every product is 2^66, past 64 bits
  {
    ffm_metrics m{};
    const uint64_t c = 1ull << 33;
    const uint64_t pos[2] = {c, c}, neg[2] = {c, c};
    CHECK(ffm_metrics_host::from_histogram(pos, neg, 2, 0, &m) == FFM_OK);
    // U2 = 2 * c * c + 2 * c * c = 4 c^2 of 2 P N = 8 c^2; T = 2 c^2
    CHECK(m.auc == 0.5 && m.auc_slack == 0.25 && m.n_pos == static_cast<int64_t>(2 * c) && m.n_mixed_bins == 2);
    const uint64_t pos2[2] = {0, c}, neg2[2] = {c, 3 * c};
    CHECK(ffm_metrics_host::from_histogram(pos2, neg2, 2, 0, &m) == FFM_OK);
    // U2 = 2 * c * c + 3 c^2 = 5 c^2 of 2 * c * 4c = 8 c^2; T = 3 c^2
    CHECK(m.auc == 0.625 && m.auc_slack == 0.375);
    compare({c, c, 0, c + 1}, {c - 1, 0, c, c}, 0);
  }
  // an empty class: NaN, still a success; so is no bin at all
  {
    ffm_metrics m{};
    const uint64_t some[3] = {1, 2, 3}, none[3] = {0, 0, 0};
    CHECK(ffm_metrics_host::from_histogram(some, none, 3, 4, &m) == FFM_OK);
    CHECK(std::isnan(m.auc) && std::isnan(m.auc_slack) && m.n_pos == 6 && m.n_neg == 0 && m.n_nan == 4);
    CHECK(ffm_metrics_host::from_histogram(none, some, 3, 0, &m) == FFM_OK);
    CHECK(std::isnan(m.auc) && m.n_neg == 6);
    CHECK(ffm_metrics_host::from_histogram(nullptr, nullptr, 0, 0, &m) == FFM_OK);
    CHECK(std::isnan(m.auc) && m.n_pos == 0 && m.n_neg == 0);
  }
  // the engine's size, sparse: 2^20 bins, a few thousand of them filled (linear-time restatement)
  {
    const size_t n = static_cast<size_t>(FFM_METRIC_BINS);
    std::vector<uint64_t> pos(n, 0), neg(n, 0);
    for (int i = 0; i < 4000; i++) {
      pos[rng() % n] += rng() % 1000;
      neg[rng() % n] += rng() % 1000;
    }
    pos[n - 1] += 17;
    neg[0] += 5;
    u128 below = 0, ties = 0, P = 0, N = 0;
    for (size_t b = 0; b < n; b++) {
      below += static_cast<u128>(pos[b]) * N;
      ties += static_cast<u128>(pos[b]) * neg[b];
      P += pos[b];
      N += neg[b];
    }
    ffm_metrics m{};
    CHECK(ffm_metrics_host::from_histogram(pos.data(), neg.data(), static_cast<int64_t>(n), 0, &m) == FFM_OK);
    CHECK(m.n_pos == static_cast<int64_t>(P) && m.n_neg == static_cast<int64_t>(N));
    CHECK(m.auc == static_cast<double>(2 * below + ties) / static_cast<double>(2 * P * N));
    CHECK(m.auc_slack == static_cast<double>(ties) / static_cast<double>(2 * P * N));
  }
  // refused arguments
  {
    ffm_metrics m{};
    const uint64_t one = 1;
    CHECK(ffm_metrics_host::from_histogram(&one, &one, 1, 0, nullptr) == FFM_E_INVALID);
    CHECK(ffm_metrics_host::from_histogram(nullptr, &one, 1, 0, &m) == FFM_E_INVALID);
    CHECK(ffm_metrics_host::from_histogram(&one, nullptr, 1, 0, &m) == FFM_E_INVALID);
    CHECK(ffm_metrics_host::from_histogram(&one, &one, -1, 0, &m) == FFM_E_INVALID);
    CHECK(ffm_metrics_host::from_histogram(&one, &one, 1, -1, &m) == FFM_E_INVALID);
  }
  std::printf("%d checks, %d failed\n", n_checks, n_failed);
  return n_failed ? 1 : 0;
}
