// kernels_metric.h -- the score histogram behind the AUC channels (include/ffm_engine.h "Metrics").
//
// One lane per labelled row: p = sigmoid_ref(logit) (the bits predict(..., output_prob = 1) returns),
// bin(p) = min((int)(p * 2^20), 2^20 - 1), and the row counts once in pos[bin] (label > 0) or
// neg[bin].  A NaN score goes into no bin and counts in *n_nan.  The counters are 64-bit integers, so
// the histogram does not depend on the order the rows arrive in: integer atomics, no float atomics.
//
// The lanes of a wave that share a (bin, class) key are added by ONE atomic: on a fresh model every
// row has p = 0.5 exactly, which would otherwise be 8192 atomics on one address per block.  Each turn
// of the loop takes the key of the first lane still waiting, ballots the lanes that carry it, lets
// that first lane add their number, and retires them; a wave whose 64 rows fall into 64 bins takes 64
// turns of a few scalar instructions each.  The key is (bin, class), not the bin: rows of both
// labels in one bin go to two different counters.  No LDS, no barrier.
#pragma once
#include "engine_types.h"
#include "ftrl_math.h"

namespace ftrl_dev {

constexpr int kMetricThreads = 256;
constexpr int kMetricBins = 1 << 20;  // FFM_METRIC_BINS

// (the clamps are no-ops for every p a sigmoid returns, [0, 1]; they keep any other float inside the
// arrays.  p * 2^20 is exact, the conversion truncates; min in float first is the same bin as min
// after the conversion, because 2^20 - 1 is a float.)
__device__ __forceinline__ int metric_bin(float p) {
  return static_cast<int>(fmaxf(fminf(p * 1048576.0f, 1048575.0f), 0.0f));
}

__global__ __launch_bounds__(kMetricThreads) void metric_hist_kernel(int n_rows, const float *score, int is_prob,
                                                                     const int *label, unsigned long long *pos,
                                                                     unsigned long long *neg, unsigned long long *n_nan) {
  const int r = blockIdx.x * kMetricThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  float p = 0.0f;
  int cls = 0;
  const bool live = r < n_rows;
  if (live) {
    const float s = score[r];
    p = is_prob ? s : sigmoid_ref(s);
    cls = label[r] > 0 ? 1 : 0;
  }
  const bool is_nan = live && p != p;
  const unsigned long long nan_mask = __ballot(is_nan);
  if (nan_mask != 0ull && lane == __ffsll(nan_mask) - 1)
    __hip_atomic_fetch_add(n_nan, static_cast<unsigned long long>(__popcll(nan_mask)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const bool counts = live && !is_nan;
  const int key = counts ? metric_bin(p) * 2 + cls : -1;
  unsigned long long waiting = __ballot(counts);  // (wave-uniform: every lane walks the same turns)
  while (waiting != 0ull) {
    const int first = __ffsll(waiting) - 1;
    const int k0 = __builtin_amdgcn_readlane(key, first);  // the first waiting lane's key
    const unsigned long long same = __ballot(key == k0);
    if (lane == first)
      __hip_atomic_fetch_add(((k0 & 1) ? pos : neg) + (k0 >> 1), static_cast<unsigned long long>(__popcll(same)),
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    waiting &= ~same;
  }
}

}  // namespace ftrl_dev
