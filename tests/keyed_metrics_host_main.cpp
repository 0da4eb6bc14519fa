// keyed_metrics_host_main.cpp -- stand-alone check of csrc/metrics_host.h's grouped AUC (per-key table ->
// GAUC): built by tests/test_keyed_metrics_host.py with g++ alone, plainly and with
// -fsanitize=address,undefined, and run directly.  Tables are made from rows by a pair-by-pair count
// (quadratic), reduced by from_keyed, and compared with the header's formula spelled out once more and with
// closed forms; the shape and argument checks the engine's refusals use are exercised without a device.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#include "../ftrl-ffm_amd/csrc/metrics_host.h"

static int n_checks = 0, n_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    n_checks++;                                                            \
    if (!(cond)) {                                                         \
      n_failed++;                                                          \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
    }                                                                      \
  } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0 || (std::isnan(a) && std::isnan(b)); }

struct Row { int key; float p; int cls; };
struct Table { std::vector<int64_t> pos, neg; std::vector<uint64_t> u2; };

// P, N, U2 of every key by looking at every pair of its rows
static Table brute(const std::vector<Row> &rows) {
  std::map<int, std::vector<Row>> by_key;
  for (const Row &r : rows) by_key[r.key].push_back(r);
  Table t;
  for (const auto &kv : by_key) {
    int64_t P = 0, N = 0;
    uint64_t u2 = 0;
    for (const Row &a : kv.second) {
      (a.cls ? P : N)++;
      if (!a.cls) continue;
      for (const Row &b : kv.second)
        if (!b.cls) u2 += b.p < a.p ? 2 : b.p == a.p ? 1 : 0;
    }
    t.pos.push_back(P);
    t.neg.push_back(N);
    t.u2.push_back(u2);
  }
  return t;
}

// the header's order of operations, once more
static ffm_keyed_metrics spelled(const Table &t) {
  ffm_keyed_metrics m{};
  double num = 0.0, den = 0.0;
  for (size_t g = 0; g < t.pos.size(); g++) {
    m.n_rows += t.pos[g] + t.neg[g];
    if (t.pos[g] == 0 || t.neg[g] == 0) continue;
    const double auc = static_cast<double>(t.u2[g]) / (2.0 * static_cast<double>(t.pos[g]) * static_cast<double>(t.neg[g]));
    num += static_cast<double>(t.pos[g] + t.neg[g]) * auc;
    den += static_cast<double>(t.pos[g] + t.neg[g]);
    m.n_keys_mixed++;
    m.n_rows_mixed += t.pos[g] + t.neg[g];
  }
  m.n_keys = static_cast<int64_t>(t.pos.size());
  m.gauc = den == 0.0 ? NAN : num / den;
  return m;
}

static ffm_keyed_metrics reduce(const Table &t, int *rc) {
  ffm_keyed_metrics m;
  std::memset(&m, 0x5a, sizeof m);  // (every field must be written)
  *rc = ffm_metrics_host::from_keyed(t.pos.data(), t.neg.data(), t.u2.data(), static_cast<int64_t>(t.pos.size()), &m);
  return m;
}

static void compare(const Table &t) {
  int rc = -99;
  const ffm_keyed_metrics got = reduce(t, &rc), want = spelled(t);
  CHECK(rc == FFM_OK);
  CHECK(got.n_rows == want.n_rows && got.n_keys == want.n_keys && got.n_keys_mixed == want.n_keys_mixed &&
        got.n_rows_mixed == want.n_rows_mixed);
  CHECK(got.n_nan == 0 && got.n_unkeyed == 0 && got.n_overflow == 0);
  CHECK(same_bits(got.gauc, want.gauc));
  if (!std::isnan(got.gauc)) CHECK(got.gauc >= 0.0 && got.gauc <= 1.0);
}

int main() {
  static_assert(sizeof(ffm_keyed_metrics) == 64, "seven counts and a double");
  std::mt19937_64 rng(31);
  // random rows: few keys and many, few distinct scores (ties) and many
  for (int n_rows : {1, 2, 7, 64, 300}) {
    for (int rep = 0; rep < 8; rep++) {
      const int n_keys = rep & 1 ? 3 : 40, n_scores = rep & 2 ? 4 : 1000;
      std::vector<Row> rows(n_rows);
      for (Row &r : rows)
        r = Row{static_cast<int>(rng() % n_keys), static_cast<float>(rng() % n_scores) / static_cast<float>(n_scores),
                static_cast<int>(rng() % 10 < (rep & 4 ? 5 : 2))};
      compare(brute(rows));
    }
  }
  // one key, perfectly separated both ways round, and all ties
  {
    int rc;
    ffm_keyed_metrics m = reduce(brute({{5, 0.1f, 0}, {5, 0.2f, 0}, {5, 0.7f, 1}}), &rc);
    CHECK(rc == FFM_OK && m.gauc == 1.0 && m.n_keys == 1 && m.n_keys_mixed == 1 && m.n_rows == 3 && m.n_rows_mixed == 3);
    m = reduce(brute({{5, 0.9f, 0}, {5, 0.8f, 0}, {5, 0.7f, 1}}), &rc);
    CHECK(rc == FFM_OK && m.gauc == 0.0);
    const Table ties{{12}, {30}, {12 * 30}};  // U2 = P * N
    m = reduce(ties, &rc);
    CHECK(rc == FFM_OK && m.gauc == 0.5 && m.n_rows == 42);
    const Table two{{12, 3}, {30, 3}, {12 * 30, 18}};  // 0.5 and 1.0, weighted 42 : 6
    m = reduce(two, &rc);
    CHECK(rc == FFM_OK && same_bits(m.gauc, (42.0 * 0.5 + 6.0 * 1.0) / 48.0));
  }
  // no mixed key: NaN, still a success; so is no key at all
  {
    int rc;
    ffm_keyed_metrics m = reduce(Table{{4, 0, 2}, {0, 9, 0}, {0, 0, 0}}, &rc);
    CHECK(rc == FFM_OK && std::isnan(m.gauc) && m.n_keys == 3 && m.n_keys_mixed == 0 && m.n_rows == 15 && m.n_rows_mixed == 0);
    ffm_keyed_metrics z;
    CHECK(ffm_metrics_host::from_keyed(nullptr, nullptr, nullptr, 0, &z) == FFM_OK);
    CHECK(std::isnan(z.gauc) && z.n_keys == 0 && z.n_rows == 0);
  }
  // P, N near 2^31: 2 P N passes 2^63 as an integer, not as a double
  {
    int rc;
    const int64_t P = (1ll << 31) + 5, N = (1ll << 31) + 1;
    const uint64_t pn = static_cast<uint64_t>(P) * static_cast<uint64_t>(N);  // just above 2^62
    ffm_keyed_metrics m = reduce(Table{{P}, {N}, {pn}}, &rc);
    CHECK(rc == FFM_OK && m.gauc == static_cast<double>(pn) / (2.0 * static_cast<double>(P) * static_cast<double>(N)));
    CHECK(std::fabs(m.gauc - 0.5) < 1e-15 && m.n_rows == P + N);
    m = reduce(Table{{P, 1}, {N, 1}, {2 * pn, 0}}, &rc);  // U2 = 2 P N: past 2^63 as a signed integer
    CHECK(rc == FFM_OK && m.gauc > 0.999999999 && m.gauc <= 1.0 && m.n_keys_mixed == 2);
    compare(Table{{P, 7, P - 5}, {N, 1, 3}, {pn, 9, static_cast<uint64_t>(P - 5) * 5}});
  }
  // refused arguments
  {
    ffm_keyed_metrics m{};
    const int64_t one = 1, minus = -1;
    const uint64_t u = 1;
    CHECK(ffm_metrics_host::from_keyed(&one, &one, &u, 1, nullptr) == FFM_E_INVALID);
    CHECK(ffm_metrics_host::from_keyed(nullptr, &one, &u, 1, &m) == FFM_E_INVALID);
    CHECK(ffm_metrics_host::from_keyed(&one, nullptr, &u, 1, &m) == FFM_E_INVALID);
    CHECK(ffm_metrics_host::from_keyed(&one, &one, nullptr, 1, &m) == FFM_E_INVALID);
    CHECK(ffm_metrics_host::from_keyed(&one, &one, &u, -1, &m) == FFM_E_INVALID);
    CHECK(ffm_metrics_host::from_keyed(&minus, &one, &u, 1, &m) == FFM_E_INVALID);
    CHECK(ffm_metrics_host::from_keyed(&one, &minus, &u, 1, &m) == FFM_E_INVALID);
  }
  // what the engine refuses from its config alone, with no device anywhere near
  {
    using namespace ffm_metrics_host;
    CHECK(keyed_shape_check(FFM_MODEL_FFM, 1, false) == FFM_OK);
    CHECK(keyed_shape_check(FFM_MODEL_LR, 1, false) == FFM_E_UNSUPPORTED);
    CHECK(keyed_shape_check(FFM_MODEL_FM, 1, false) == FFM_E_UNSUPPORTED);
    CHECK(keyed_shape_check(FFM_MODEL_FFM, 2, false) == FFM_E_UNSUPPORTED);
    CHECK(keyed_shape_check(FFM_MODEL_FFM, 1, true) == FFM_E_UNSUPPORTED);
    CHECK(keyed_args_check(4, 0, 1) == FFM_OK && keyed_args_check(4, 3, 1ll << 24) == FFM_OK);
    CHECK(keyed_args_check(4, -1, 1) == FFM_E_INVALID && keyed_args_check(4, 4, 1) == FFM_E_INVALID);
    CHECK(keyed_args_check(4, 0, 0) == FFM_E_INVALID && keyed_args_check(4, 0, -5) == FFM_E_INVALID);
  }
  std::printf("%d checks, %d failed\n", n_checks, n_failed);
  return n_failed ? 1 : 0;
}
