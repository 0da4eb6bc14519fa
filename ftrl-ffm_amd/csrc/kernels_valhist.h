// kernels_valhist.h -- value buckets (include/ffm_engine.h "Value buckets"): how often every (field, bin) of a
// numeric column occurs, counted from rows in page-locked host memory (or in HBM) before a model exists; and the
// in-place mapping of an engine that holds a bucket table.  Host side: engine_valhist.h.  (The upload kernel's
// bucketing variants: kernels_stage.h; the mapping of one entry: hash_ids.h.)
//
// valhist_kernel walks its entries as every counting kernel does (count_walk, kernels_count.h).
// The histogram is n_fields x 65536 64-bit words in HBM.  The hazard is skew -- half of a count column is one
// value -- so a workgroup sums in LDS first: a write-back cache of kValhistSets sets of two ways.  A way is ONE
// 64-bit word, key << 32 | count, the key being field << 16 | bin (the word's index in the histogram) and an
// empty way all ones.  Every change of a way is one 64-bit LDS compare-and-swap on the whole word:
//   hit    (key, c)   -> (key, c + 1)
//   fill   empty      -> (key, 1)
//   evict  (other, c) -> (key, 1), and the lane whose swap succeeded adds c to other's word in HBM
// A failed swap is tried again on what it found.  Whoever removes a word adds exactly its count, and the words
// left at the end are added by the flush behind the barrier, so every entry is counted once whatever the
// interleaving: integer sums only, exact.  An entry whose key sits in neither way of its set and finds no
// empty one evicts the way with the smaller count (a plain read: a heuristic, never a correctness matter), so of
// two hot keys in one set both stay.  Global atomics per entry: one per eviction plus the final flush -- for a
// column of D distinct bins per workgroup at most D when D <= the cache, and for the hot value one per
// workgroup.  n_valid / n_bad / n_nan: the walk's ballots, one atomic per wave.  No float instruction touches a value.
#pragma once
#include "kernels_count.h"

namespace ftrl_dev {

constexpr unsigned kValhistSets = 1024;  // x 2 ways x 8 bytes = 16 KB of LDS
// The set of a key: the top 10 bits of a multiplicative hash (tests/test_gpu_value_buckets.py builds keys that share one).
__device__ __forceinline__ unsigned valhist_set(unsigned key) { return (key * 0x9e3779b1u) >> 22; }

__device__ __forceinline__ void valhist_flush(unsigned long long word, unsigned long long *hist) {
  __hip_atomic_fetch_add(hist + (word >> 32), word & 0xffffffffull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One counting entry into the workgroup's cache.
__device__ __forceinline__ void valhist_count(unsigned key, unsigned long long *cache, unsigned long long *hist) {
  const unsigned long long kEmpty = ~0ull, mine = static_cast<unsigned long long>(key) << 32;
  unsigned long long *way = cache + 2u * valhist_set(key);
  for (;;) {
    const unsigned long long w0 = __hip_atomic_load(way, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    const unsigned long long w1 = __hip_atomic_load(way + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    unsigned pick;
    unsigned long long seen, next;
    if ((w0 >> 32) == key) pick = 0u;
    else if ((w1 >> 32) == key) pick = 1u;
    else if (w0 == kEmpty) pick = 0u;
    else if (w1 == kEmpty) pick = 1u;
    else pick = (w1 & 0xffffffffull) < (w0 & 0xffffffffull) ? 1u : 0u;
    seen = pick ? w1 : w0;
    next = (seen >> 32) == key ? seen + 1ull : (mine | 1ull);
    if (atomicCAS(way + pick, seen, next) == seen) {
      if (seen != kEmpty && (seen >> 32) != key) valhist_flush(seen, hist);
      return;
    }
  }
}

// One entry: 0 = bad field, 1 = counted, 2 = a counting NaN.
__device__ __forceinline__ unsigned valhist_entry(unsigned F, int field, unsigned vbits, unsigned long long *cache, unsigned long long *hist) {
  if (static_cast<unsigned>(field) >= F) return 0u;
  if (ftrl_hash::value_is_nan(vbits)) return 2u;
  valhist_count((static_cast<unsigned>(field) << 16) | ftrl_hash::value_bin(vbits), cache, hist);
  return 1u;
}

// Entries [0, nnz) of a call, walked by count_walk (kernels_count.h) between the cache's set-up and its flush.
// hist: F x 65536 words.  counters: n_valid, n_bad, n_nan.
template <bool HAS_FIELD>
__global__ __launch_bounds__(256) void valhist_kernel(unsigned nnz, const int *field, const unsigned *val, unsigned first, unsigned F,
                                                      int vec, unsigned long long *hist, unsigned long long *counters) {
  __shared__ unsigned long long cache[2 * kValhistSets];
  for (unsigned i = threadIdx.x; i < 2 * kValhistSets; i += blockDim.x) cache[i] = ~0ull;
  __syncthreads();
  count_walk<HAS_FIELD, false, true>(nnz, field, val, first, F, vec, counters,
                                     [&](int fld, unsigned vbits) { return valhist_entry(F, fld, vbits, cache, hist); });
  // the flush: every wave of the workgroup is past its last swap
  __syncthreads();
  for (unsigned i = threadIdx.x; i < 2 * kValhistSets; i += blockDim.x) {
    const unsigned long long w = cache[i];
    if (w != ~0ull) valhist_flush(w, hist);
  }
}

// hash_ids_rare_kernel (kernels_idcount.h) for an FFM engine with a bucket table: the same loops, and val moves
// with feat -- a bucketed entry becomes (bucket, 1.0f) and is hashed, every other entry is folded (rare.words !=
// nullptr) and hashed as before and keeps its value (ftrl_hash::hash_entry_bucket).  In place (feat_out ==
// feat_in, val_out == val_in) is fine: a lane reads its entries before it writes them.  A kernel of its own, so
// that an engine without a table runs the kernels it always ran.
__global__ __launch_bounds__(256) void hash_ids_bucket_kernel(ftrl_hash::Map hm, ftrl_hash::Rare rare, ftrl_hash::Buckets bk, unsigned nnz,
                                                              const int *field, const int *feat_in, int *feat_out,
                                                              const unsigned *val_in, unsigned *val_out, int vec) {
  const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  const unsigned n4 = vec ? nnz >> 2 : 0u, F = static_cast<unsigned>(hm.n_fields);
  for (unsigned i = tid; i < n4; i += stride) {
    const int4 ft = reinterpret_cast<const int4 *>(feat_in)[i];
    const int4 fl = field ? reinterpret_cast<const int4 *>(field)[i] : ftrl_hash::hash_implicit_fields4(i, F);
    uint4 v = reinterpret_cast<const uint4 *>(val_in)[i];
    reinterpret_cast<int4 *>(feat_out)[i] = ftrl_hash::hash_entries4_bucket(hm, rare, bk, fl, ft, &v);
    reinterpret_cast<uint4 *>(val_out)[i] = v;
  }
  for (unsigned p = (n4 << 2) + tid; p < nnz; p += stride) {
    unsigned v = val_in[p];
    feat_out[p] = ftrl_hash::hash_entry_bucket(hm, rare, bk, field ? field[p] : static_cast<int>(p % F), feat_in[p], &v);
    val_out[p] = v;
  }
}

}  // namespace ftrl_dev
