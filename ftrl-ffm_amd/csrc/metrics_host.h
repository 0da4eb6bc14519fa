// metrics_host.h -- from a score histogram to AUC, on the host, in exact integer arithmetic
// (include/ffm_engine.h "Metrics": ffm_engine_metrics_from_histogram and ffm_engine_metrics_read); and from a
// per-key table to the grouped AUC (from_keyed below: ffm_engine_metrics_from_keyed and _read_keyed).
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

// From a per-key table to the grouped AUC (include/ffm_engine.h "Metrics", keyed capture:
// ffm_engine_metrics_from_keyed and ffm_engine_metrics_read_keyed).  pos / neg / u2 of key g as the
// device's rank pass leaves them, keys ascending.  The counts are exact integers; the average is taken
// in double, one running sum each, in the order the header states -- so every caller that follows that
// order gets the same bits.  2 * P_g * N_g is formed in double: it passes 2^63 as an integer long before
// it loses a bit as a double's product of two counts below 2^31.
// Refused: a null output, a negative n_keys, a null array with n_keys > 0, a negative count.
// n_nan, n_unkeyed and n_overflow are not the table's to know: they are set to 0 here.
inline int from_keyed(const int64_t *pos, const int64_t *neg, const uint64_t *u2, int64_t n_keys, ffm_keyed_metrics *out) {
  if (!out || n_keys < 0 || (n_keys > 0 && (!pos || !neg || !u2))) return FFM_E_INVALID;
  for (int64_t g = 0; g < n_keys; g++)
    if (pos[g] < 0 || neg[g] < 0) return FFM_E_INVALID;
  int64_t n_rows = 0, n_mixed = 0, n_rows_mixed = 0;
  double num = 0.0, den = 0.0;
  for (int64_t g = 0; g < n_keys; g++) {
    const int64_t P = pos[g], N = neg[g];
    n_rows += P + N;
    if (P == 0 || N == 0) continue;
    const double auc_g = static_cast<double>(u2[g]) / (2.0 * static_cast<double>(P) * static_cast<double>(N));
    num += static_cast<double>(P + N) * auc_g;
    den += static_cast<double>(P + N);
    n_mixed++;
    n_rows_mixed += P + N;
  }
  out->n_rows = n_rows;
  out->n_keys = n_keys;
  out->n_keys_mixed = n_mixed;
  out->n_rows_mixed = n_rows_mixed;
  out->n_nan = out->n_unkeyed = out->n_overflow = 0;
  out->gauc = den == 0.0 ? NAN : num / den;
  return FFM_OK;
}

// Whether keyed capture applies to an engine of this shape, from its config alone (no device): FFM only
// (LR and FM have no fields), one shard, not inside a group.  FFM_OK or FFM_E_UNSUPPORTED.
inline int keyed_shape_check(int32_t model_type, int32_t n_shards, bool in_group) {
  return model_type == FFM_MODEL_FFM && n_shards == 1 && !in_group ? FFM_OK : FFM_E_UNSUPPORTED;
}
// ... and its two arguments: the key field names a field, the capacity is positive.
inline int keyed_args_check(int32_t n_fields, int32_t key_field, int64_t capacity_rows) {
  return key_field >= 0 && key_field < n_fields && capacity_rows > 0 ? FFM_OK : FFM_E_INVALID;
}

}  // namespace ffm_metrics_host
