// kernels_count.h -- the walk the counting kernels share (field_sketch_kernel, kernels_sketch.h; idcount_kernel,
// kernels_idcount.h; valhist_kernel, kernels_valhist.h).  It has the shape of pull_block_kernel (kernels_stage.h):
// few workgroups when it reads over PCIe, a lane loads the int4 of field and the 16 bytes of the second array (feat
// or val) over a grid stride, what is left goes entry by entry.  n_valid / n_bad (/ n_nan): every wave adds its
// ballots' popcounts in wave-uniform counters and issues one integer atomic each at its end (as metric_hist_kernel
// counts NaNs) -- integer sums only, so they do not depend on the order or the batching of the entries.
#pragma once
#include "hash_ids.h"

namespace ftrl_dev {

// Entries [0, nnz) of a call.  field / second: device-visible; vec != 0: both are 16-byte aligned.  HAS_FIELD ==
// false: entry p of the call is field (first + p) mod F, first a multiple of 4 (a call cut into chunks) -- or, where
// ZERO_F_IS_FIELD_0 (idcount_kernel alone: LR / FM), field 0 when F == 0.  entry(field, bits of the second array's
// element): 0 = not counted, 1 = counted, 2 = a counted NaN (HAS_NAN only).  counters: n_valid, n_bad, and n_nan
// where HAS_NAN.  Every loop is wave-uniform (a lane past the end idles): the ballots see whole waves.
// block_dim / grid_dim: never passed -- the defaults are evaluated in the calling kernel, where the compiler knows that
// all workgroups have the same size; read in here they cost a select per launch and a register or two.
template <bool HAS_FIELD, bool ZERO_F_IS_FIELD_0, bool HAS_NAN, typename Entry>
__device__ __forceinline__ void count_walk(unsigned nnz, const int *field, const unsigned *second, unsigned first, unsigned F, int vec,
                                           unsigned long long *counters, Entry entry,
                                           unsigned block_dim = blockDim.x, unsigned grid_dim = gridDim.x) {
  using R = decltype(entry(0, 0u));  // (bool where !HAS_NAN)
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");  // (a refilled page-locked buffer: pull_block_kernel's reason)
  const unsigned lane = threadIdx.x & 63u;
  const unsigned wave0 = blockIdx.x * block_dim + threadIdx.x - lane, stride = grid_dim * block_dim;
  const unsigned n4 = vec ? nnz >> 2 : 0u;
  unsigned n_ok = 0, n_seen = 0;  // wave-uniform
  [[maybe_unused]] unsigned n_nan = 0;
  for (unsigned base = wave0; base < n4; base += stride) {
    const unsigned i = base + lane;
    const bool live = i < n4;
    R r0{}, r1{}, r2{}, r3{};
    if (live) {
      const uint4 v = reinterpret_cast<const uint4 *>(second)[i];
      int4 fl;
      if constexpr (HAS_FIELD) fl = reinterpret_cast<const int4 *>(field)[i];
      else if constexpr (ZERO_F_IS_FIELD_0) fl = F ? ftrl_hash::hash_implicit_fields4((first >> 2) + i, F) : make_int4(0, 0, 0, 0);
      else fl = ftrl_hash::hash_implicit_fields4((first >> 2) + i, F);
      r0 = entry(fl.x, v.x);
      r1 = entry(fl.y, v.y);
      r2 = entry(fl.z, v.z);
      r3 = entry(fl.w, v.w);
    }
    n_ok += __popcll(__ballot(r0 != R{})) + __popcll(__ballot(r1 != R{})) + __popcll(__ballot(r2 != R{})) + __popcll(__ballot(r3 != R{}));
    if constexpr (HAS_NAN)
      n_nan += __popcll(__ballot(r0 == 2u)) + __popcll(__ballot(r1 == 2u)) + __popcll(__ballot(r2 == 2u)) + __popcll(__ballot(r3 == 2u));
    n_seen += 4u * __popcll(__ballot(live));
  }
  for (unsigned base = (n4 << 2) + wave0; base < nnz; base += stride) {
    const unsigned p = base + lane;
    const bool live = p < nnz;
    R r{};
    if (live) {
      int f;
      if constexpr (HAS_FIELD) f = field[p];
      else if constexpr (ZERO_F_IS_FIELD_0) f = F ? static_cast<int>((first % F + p % F) % F) : 0;
      else f = static_cast<int>((first % F + p % F) % F);
      r = entry(f, second[p]);
    }
    n_ok += __popcll(__ballot(r != R{}));
    if constexpr (HAS_NAN) n_nan += __popcll(__ballot(r == 2u));
    n_seen += __popcll(__ballot(live));
  }
  if (lane == 0u) {
    if (n_ok) __hip_atomic_fetch_add(counters, static_cast<unsigned long long>(n_ok), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n_seen != n_ok)
      __hip_atomic_fetch_add(counters + 1, static_cast<unsigned long long>(n_seen - n_ok), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if constexpr (HAS_NAN)
      if (n_nan) __hip_atomic_fetch_add(counters + 2, static_cast<unsigned long long>(n_nan), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace ftrl_dev
