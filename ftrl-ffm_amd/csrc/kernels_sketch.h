// kernels_sketch.h -- field sketches (include/ffm_engine.h "Field sketches"): one HyperLogLog sketch per field,
// filled from rows in page-locked host memory (or in HBM) before a model exists, so that the fields' id ranges
// can be sized by what the fields hold.  Host side: engine_sketch.h.
//
// The kernel walks its entries as every counting kernel does (count_walk, kernels_count.h).  The hashed bits are
// those hash_into scales (csrc/hash_ids.h), so the integer work hides behind the link.
// Registers are 32-bit words in HBM.  Per counting entry: a plain load of its register, and an atomic max only
// when the entry's rank exceeds what was loaded.  Registers only grow, so a stale load can cause a superfluous
// atomic and never a missed one -- after the first blocks the Zipf head's entries stop issuing atomics at all.
// n_valid / n_bad: the walk's ballots.  No LDS, no barrier, no float atomics; maxima and integer sums only, so
// the result does not depend on the order or the batching of the entries.
#pragma once
#include "kernels_count.h"

namespace ftrl_dev {

constexpr unsigned kSketchBits = 14, kSketchRegs = 1u << kSketchBits;  // FFM_SKETCH_REGS

// One entry: true iff it counts (feat >= 0 and 0 <= field < F -- what ftrl_hash::hash_entry keeps for FFM).
__device__ __forceinline__ bool sketch_entry(unsigned F, int field, int feat, unsigned *reg) {
  if (feat < 0 || static_cast<unsigned>(field) >= F) return false;
  const unsigned x = ftrl_hash::hash_bits(field, feat);
  const unsigned w = x << kSketchBits;
  const unsigned rank = w == 0u ? 33u - kSketchBits : static_cast<unsigned>(__clz(w)) + 1u;
  unsigned *r = reg + static_cast<size_t>(field) * kSketchRegs + (x >> (32u - kSketchBits));
  if (*r < rank) __hip_atomic_fetch_max(r, rank, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

// Entries [0, nnz) of a call, walked by count_walk (kernels_count.h).  reg: F x kSketchRegs words.  counters:
// n_valid, n_bad.
// FILTERED (ffm_engine_sketch_set_filter): one more argument, the keep-map of "Rare ids" -- an entry whose bit
// there is 0 counts as the one id kRareId of its field (ftrl_hash::fold_entry).  An instantiation of its own:
// the unfiltered kernel keeps its arguments and its instructions.
template <bool HAS_FIELD, bool FILTERED, typename... Filter>
__global__ __launch_bounds__(256) void field_sketch_kernel(unsigned nnz, const int *field, const int *feat, unsigned first,
                                                           unsigned F, int vec, unsigned *reg, unsigned long long *counters,
                                                           Filter... filter) {
  static_assert(sizeof...(Filter) == (FILTERED ? 1 : 0), "Filter: nothing, or <ftrl_hash::Rare>");
  count_walk<HAS_FIELD, false, false>(nnz, field, reinterpret_cast<const unsigned *>(feat), first, F, vec, counters, [&](int fld, unsigned bits) {
    int ft = static_cast<int>(bits);
    if constexpr (FILTERED) ft = ftrl_hash::fold_entry(true, static_cast<int>(F), filter..., fld, ft);
    return sketch_entry(F, fld, ft, reg);
  });
}

}  // namespace ftrl_dev
