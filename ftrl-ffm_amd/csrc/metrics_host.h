// metrics_host.h -- from a score histogram to AUC, on the host, in exact integer arithmetic
// (include/ffm_engine.h "Metrics": ffm_engine_metrics_from_histogram and ffm_engine_metrics_read).
//
// No HIP include and no dependency beyond the C ABI header: a stand-alone program can compile it
// (tests/metrics_host_main.cpp does, plainly and under the address / undefined-behaviour sanitizers).
//
//   P = sum pos_b, N = sum neg_b
//   T  = sum_b pos_b * neg_b                       the mixed-bin tie mass
//   U2 = 2 * sum_b pos_b * (sum_{c<b} neg_c) + T   twice the Mann-Whitney U with in-bin pairs counted 1/2
//   auc = U2 / (2 P N), auc_slack = T / (2 P N); both NaN when P * N == 0
// Counts may exceed 2^32, so the products exceed 2^64: the sums run in an unsigned 128-bit
// accumulator (exact while P and N stay below 2^63, i.e. always), and only the two final quotients
// are floating point -- two conversions and one divide each, every one correctly rounded.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/ffm_engine.h"

namespace ffm_metrics_host {

inline int from_histogram(const uint64_t *pos, const uint64_t *neg, int64_t n_bins, int64_t n_nan,
                          ffm_metrics *out) {
  if (!out || n_bins < 0 || n_nan < 0 || (n_bins > 0 && (!pos || !neg))) return FFM_E_INVALID;
  typedef unsigned __int128 u128;
  u128 below = 0, ties = 0;  // sum_b pos_b * N_{<b} and T
  uint64_t P = 0, N = 0;
  int64_t mixed = 0;
  for (int64_t b = 0; b < n_bins; b++) {
    const uint64_t p = pos[b], n = neg[b];
    if (p) below += static_cast<u128>(p) * N;
    if (p && n) {
      ties += static_cast<u128>(p) * n;
      mixed++;
    }
    P += p;
    N += n;
  }
  out->n_pos = static_cast<int64_t>(P);
  out->n_neg = static_cast<int64_t>(N);
  out->n_nan = n_nan;
  out->n_mixed_bins = mixed;
  if (P == 0 || N == 0) {
    out->auc = NAN;
    out->auc_slack = NAN;
    return FFM_OK;
  }
  const u128 u2 = 2 * below + ties, denom = 2 * (static_cast<u128>(P) * N);
  out->auc = static_cast<double>(u2) / static_cast<double>(denom);
  out->auc_slack = static_cast<double>(ties) / static_cast<double>(denom);
  return FFM_OK;
}

}  // namespace ffm_metrics_host
