// kernels_sketch.h -- field sketches (include/ffm_engine.h "Field sketches"): one HyperLogLog sketch per field,
// filled from rows in page-locked host memory (or in HBM) before a model exists, so that the fields' id ranges
// can be sized by what the fields hold.  Host side: engine_sketch.h.
//
// The kernel has the shape of pull_block_kernel (kernels_stage.h): few workgroups when it reads over PCIe, a
// lane loads the int4 of feat and the int4 of field over a grid stride, what is left goes entry by entry.  The
// hashed bits are those hash_into scales (csrc/hash_ids.h), so the integer work hides behind the link.
// Registers are 32-bit words in HBM.  Per counting entry: a plain load of its register, and an atomic max only
// when the entry's rank exceeds what was loaded.  Registers only grow, so a stale load can cause a superfluous
// atomic and never a missed one -- after the first blocks the Zipf head's entries stop issuing atomics at all.
// n_valid / n_bad: every wave adds its ballots' popcounts in a wave-uniform counter and issues one integer
// atomic each at its end (as metric_hist_kernel counts NaNs).  No LDS, no barrier, no float atomics; maxima and
// integer sums only, so the result does not depend on the order or the batching of the entries.
#pragma once
#include "hash_ids.h"

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

// Entries [0, nnz) of a call.  field / feat: device-visible; vec != 0: both are 16-byte aligned.  HAS_FIELD ==
// false: entry p of the call is field (first + p) mod F, first a multiple of 4 (a call cut into chunks).
// counters: n_valid, n_bad.  Every loop is wave-uniform (a lane past the end idles): the ballots see whole waves.
// FILTERED (ffm_engine_sketch_set_filter): one more argument, the keep-map of "Rare ids" -- an entry whose bit
// there is 0 counts as the one id kRareId of its field (ftrl_hash::fold_entry).  An instantiation of its own:
// the unfiltered kernel keeps its arguments and its instructions.
template <bool HAS_FIELD, bool FILTERED, typename... Filter>
__global__ __launch_bounds__(256) void field_sketch_kernel(unsigned nnz, const int *field, const int *feat, unsigned first,
                                                           unsigned F, int vec, unsigned *reg, unsigned long long *counters,
                                                           Filter... filter) {
  static_assert(sizeof...(Filter) == (FILTERED ? 1 : 0), "Filter: nothing, or <ftrl_hash::Rare>");
  const auto sketch_entry = [&](unsigned F_, int fld, int ft, unsigned *reg_) {
    if constexpr (FILTERED) ft = ftrl_hash::fold_entry(true, static_cast<int>(F_), filter..., fld, ft);
    return ftrl_dev::sketch_entry(F_, fld, ft, reg_);
  };
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");  // (a refilled page-locked buffer: pull_block_kernel's reason)
  const unsigned lane = threadIdx.x & 63u;
  const unsigned wave0 = blockIdx.x * blockDim.x + threadIdx.x - lane, stride = gridDim.x * blockDim.x;
  const unsigned n4 = vec ? nnz >> 2 : 0u;
  unsigned n_ok = 0, n_seen = 0;  // wave-uniform
  for (unsigned base = wave0; base < n4; base += stride) {
    const unsigned i = base + lane;
    const bool live = i < n4;
    bool ok0 = false, ok1 = false, ok2 = false, ok3 = false;
    if (live) {
      const int4 ft = reinterpret_cast<const int4 *>(feat)[i];
      int4 fl;
      if constexpr (HAS_FIELD) fl = reinterpret_cast<const int4 *>(field)[i];
      else fl = ftrl_hash::hash_implicit_fields4((first >> 2) + i, F);
      ok0 = sketch_entry(F, fl.x, ft.x, reg);
      ok1 = sketch_entry(F, fl.y, ft.y, reg);
      ok2 = sketch_entry(F, fl.z, ft.z, reg);
      ok3 = sketch_entry(F, fl.w, ft.w, reg);
    }
    n_ok += __popcll(__ballot(ok0)) + __popcll(__ballot(ok1)) + __popcll(__ballot(ok2)) + __popcll(__ballot(ok3));
    n_seen += 4u * __popcll(__ballot(live));
  }
  for (unsigned base = (n4 << 2) + wave0; base < nnz; base += stride) {
    const unsigned p = base + lane;
    const bool live = p < nnz;
    bool ok = false;
    if (live) {
      int f;
      if constexpr (HAS_FIELD) f = field[p]; else f = static_cast<int>((first % F + p % F) % F);
      ok = sketch_entry(F, f, feat[p], reg);
    }
    n_ok += __popcll(__ballot(ok));
    n_seen += __popcll(__ballot(live));
  }
  if (lane == 0u) {
    if (n_ok) __hip_atomic_fetch_add(counters, static_cast<unsigned long long>(n_ok), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n_seen != n_ok)
      __hip_atomic_fetch_add(counters + 1, static_cast<unsigned long long>(n_seen - n_ok), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace ftrl_dev
