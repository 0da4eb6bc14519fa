// kernels_idcount.h -- rare ids (include/ffm_engine.h "Rare ids"): how often every hashed slot occurs, counted
// from rows in page-locked host memory (or in HBM) before a model exists; the keep-map made of the counts; and
// the in-place hash of an engine that folds by such a map.  Host side: engine_idcount.h.  (The upload kernel's
// folding variants: kernels_stage.h; the filtered sketch: kernels_sketch.h; the fold itself: hash_ids.h.)
//
// idcount_kernel walks its entries as every counting kernel does (count_walk, kernels_count.h).  Counters are
// 32-bit words in HBM.  Per counting entry: a plain load of its word, and an integer
// atomic add only while the loaded value is below the cap.  Words only grow, so a stale load can cause a
// superfluous add and never a missed one: min(word, cap) == min(true count, cap) whatever the order, the
// batching or the split across calls -- and the Zipf head stops issuing atomics after its first `cap`
// occurrences.  (A word exceeds the cap by at most the adds in flight at once: far from 2^32.)
// n_valid / n_bad: the walk's ballots, one atomic per wave.  No LDS, no float atomics.
#pragma once
#include "kernels_count.h"

namespace ftrl_dev {

// One entry: true iff it counts (feat >= 0 and, with fields, 0 <= field < F).  F == 0: LR / FM, field taken as 0.
__device__ __forceinline__ bool idcount_entry(unsigned F, int field, int feat, unsigned shift, unsigned cap, unsigned *cnt) {
  if (feat < 0) return false;
  if (F == 0u) field = 0;
  else if (static_cast<unsigned>(field) >= F) return false;
  unsigned *c = cnt + (ftrl_hash::hash_bits(field, feat) >> shift);
  if (*c < cap) __hip_atomic_fetch_add(c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

// Entries [0, nnz) of a call, walked by count_walk (kernels_count.h); without a field array F == 0 is LR / FM, the
// field taken as 0.  cnt: 2^(32 - shift) words.  counters: n_valid, n_bad.
template <bool HAS_FIELD>
__global__ __launch_bounds__(256) void idcount_kernel(unsigned nnz, const int *field, const int *feat, unsigned first, unsigned F,
                                                      int vec, unsigned shift, unsigned cap, unsigned *cnt,
                                                      unsigned long long *counters) {
  count_walk<HAS_FIELD, true, false>(nnz, field, reinterpret_cast<const unsigned *>(feat), first, F, vec, counters, [&](int fld, unsigned bits) {
    return idcount_entry(F, fld, static_cast<int>(bits), shift, cap, cnt);
  });
}

// The keep-map of n_slots counters (a multiple of 64: bits >= 8): a lane is a slot, the ballot of
// min(count, cap) >= T is the word of the wave's 64 slots, and lane 0 stores it -- one plain 64-bit vector store.
// sums: the set bits, and the counts below T added up (T <= cap, so such a count is exact and the sum is the
// number of counted entries the map folds); per lane over the grid stride, across the wave at the end, one
// integer atomic each per wave.
__global__ __launch_bounds__(256) void idcount_keep_kernel(const unsigned *cnt, unsigned n_slots, unsigned T, unsigned cap,
                                                           unsigned long long *words, unsigned long long *sums) {
  const unsigned lane = threadIdx.x & 63u;
  const unsigned wave0 = blockIdx.x * blockDim.x + threadIdx.x - lane, stride = gridDim.x * blockDim.x;
  unsigned n_kept = 0;  // wave-uniform
  unsigned long long folded = 0;
  for (unsigned base = wave0; base < n_slots; base += stride) {
    const unsigned c = min(cnt[base + lane], cap);
    const bool keep = c >= T;
    const unsigned long long word = __ballot(keep);
    if (lane == 0u) words[base >> 6] = word;
    n_kept += __popcll(word);
    if (!keep) folded += c;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) folded += __shfl_xor(folded, d, 64);
  if (lane == 0u) {
    if (n_kept) __hip_atomic_fetch_add(sums, static_cast<unsigned long long>(n_kept), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (folded) __hip_atomic_fetch_add(sums + 1, folded, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// hash_ids_kernel (engine_hash.h) for an engine with a keep-map: the same loops, every entry folded
// (ftrl_hash::hash_entry_rare) before it is hashed.  A kernel of its own, so that an engine without a map runs
// the kernel it always ran.
__global__ __launch_bounds__(256) void hash_ids_rare_kernel(ftrl_hash::Map hm, ftrl_hash::Rare rare, unsigned nnz, const int *field,
                                                            const int *feat_in, int *feat_out, int vec) {
  const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  const unsigned n4 = vec ? nnz >> 2 : 0u, F = static_cast<unsigned>(hm.n_fields);
  for (unsigned i = tid; i < n4; i += stride) {
    const int4 ft = reinterpret_cast<const int4 *>(feat_in)[i];
    const int4 fl = field ? reinterpret_cast<const int4 *>(field)[i] : hm.ffm ? ftrl_hash::hash_implicit_fields4(i, F) : make_int4(0, 0, 0, 0);
    reinterpret_cast<int4 *>(feat_out)[i] = ftrl_hash::hash_entries4_rare(hm, rare, fl, ft);
  }
  for (unsigned p = (n4 << 2) + tid; p < nnz; p += stride)
    feat_out[p] = ftrl_hash::hash_entry_rare(hm, rare, field ? field[p] : hm.ffm ? static_cast<int>(p % F) : 0, feat_in[p]);
}

}  // namespace ftrl_dev
