// kernels_delta.h -- serving deltas (include/ffm_engine.h "Serving deltas"): a serving engine brought to a
// training engine's stored weights by a pass that COMPARES instead of copies, and rows in the table's own bits.
//   serve_sync_kernel       ffm_engine_sync_weights: per feature the target (src's lin_w bits, src's w row
//                           encoded to dst's format) against what dst stores, pattern by pattern; what differs is
//                           stored, what does not is not written; the moved features as a bitmap, three counters
//   serve_rows_raw_kernel   serve_rows_copy_kernel (kernels_serve.h) without the conversion: elements of 2 or 4 bytes
//
// serve_sync_kernel has changed_scan_kernel's shape (kernels_scan.h): one wave owns one 64-bit word of the
// bitmap = 64 consecutive features, builds it in a wave-uniform register and lane 0 stores it once with a
// vector store; no atomics, no LDS, no barriers for the bitmap.  A wave walks the words grid-stride.
//   1. lane = feature: src's and dst's lin_w, coalesced -- one ballot; a lane whose pattern differs stores it.
//   2. per feature the lanes stream the w component of src's record (16-byte non-temporal loads) and dst's row
//      (16-byte for fp32, 8-byte for fp16), kSyncU vectors of four elements per lane and chunk, all of a chunk's
//      loads issued before the first compare; a vector that differs is stored from what was loaded -- one ballot
//      per feature.  (row_len % 4 == 0: a serving engine's n_factors is a multiple of 4.)
//   3. the counters: lane-private sums, one wave reduction and one atomic per counter and wave at the end, every
//      counter on a 64-byte line of its own as in serve_pack_kernel.
// 64-bit element offsets throughout.
#pragma once
#include "kernels_serve.h"

namespace ftrl_dev {

enum { SY_MOVED = 0, SY_LIN = 1, SY_LAT = 2, SY_BIAS = 3, SY_COUNT = 4 };
constexpr int kSyncThreads = 256;
constexpr int kSyncWaves = kSyncThreads / 64;
constexpr int kSyncU = 4;  // vectors per lane in flight from either side

typedef unsigned v2u_nt __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint2 load_nt(const uint2 *p) {
  const v2u_nt v = __builtin_nontemporal_load(reinterpret_cast<const v2u_nt *>(p));
  return make_uint2(v.x, v.y);
}

// The target of four consecutive elements in the table's own bits, and how many of them differ from `have`.
__device__ __forceinline__ float4 sync_target(float4 w, float4) { return w; }
__device__ __forceinline__ uint2 sync_target(float4 w, uint2) { return serve_enc16x4(w); }
__device__ __forceinline__ unsigned sync_differ(float4 want, float4 have) {
  return (__float_as_uint(want.x) != __float_as_uint(have.x) ? 1u : 0u) + (__float_as_uint(want.y) != __float_as_uint(have.y) ? 1u : 0u) +
         (__float_as_uint(want.z) != __float_as_uint(have.z) ? 1u : 0u) + (__float_as_uint(want.w) != __float_as_uint(have.w) ? 1u : 0u);
}
__device__ __forceinline__ unsigned sync_differ(uint2 want, uint2 have) {
  const unsigned a = want.x ^ have.x, b = want.y ^ have.y;
  return ((a & 0xffffu) ? 1u : 0u) + ((a >> 16) ? 1u : 0u) + ((b & 0xffffu) ? 1u : 0u) + ((b >> 16) ? 1u : 0u);
}

// bitmap[n_words], n_words = ceil(n_feats / 64): bit (i & 63) of word i / 64 = feature i moved; bits past
// n_feats are zero.  counters: SY_COUNT sums kPackLine 64-bit words apart, zeroed by the caller.
template <int FMT>
__global__ __launch_bounds__(kSyncThreads) void serve_sync_kernel(ModelDev src, ModelDev dst, int64_t n_words,
                                                                  unsigned long long *bitmap, unsigned long long *counters) {
  static_assert(FMT == SERVE_F32 || FMT == SERVE_F16, "a packed table of w alone");
  using Raw = typename std::conditional<FMT == SERVE_F16, uint2, float4>::type;  // four elements as stored
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kSyncWaves;
  const int64_t w0 = static_cast<int64_t>(blockIdx.x) * kSyncWaves + wv;
  const int64_t RL4 = src.row_len / 4;  // vectors per row
  const float4 *const rec = reinterpret_cast<const float4 *>(src.lat);
  Raw *const table = reinterpret_cast<Raw *>(dst.lat);
  unsigned n_lin = 0u, n_lat = 0u, n_moved = 0u;  // (n_moved: the whole word's count, kept by lane 0)
  if (w0 == 0 && lane == 0) {
    const unsigned want = __float_as_uint(src.bias3[0]);
    if (want != __float_as_uint(dst.bias3[0])) {
      dst.bias3[0] = __uint_as_float(want);
      counters[SY_BIAS * kPackLine] = 1ull;  // (one writer; the caller zeroed it)
    }
  }
  for (int64_t wi = w0; wi < n_words; wi += n_waves) {
    const int64_t f0 = wi * 64;
    const int64_t fl = f0 + lane;
    bool lin_moved = false;
    if (fl < src.n_feats) {
      const float want = __builtin_nontemporal_load(src.lin_w + fl);
      lin_moved = __float_as_uint(want) != __float_as_uint(__builtin_nontemporal_load(dst.lin_w + fl));
      if (lin_moved) dst.lin_w[fl] = want;
    }
    n_lin += lin_moved ? 1u : 0u;
    unsigned long long word = __ballot(lin_moved);
    const int nf = static_cast<int>(src.n_feats - f0 < 64 ? src.n_feats - f0 : 64);
    for (int j = 0; j < nf; j++) {
      const float4 *const from = rec + (f0 + j) * 3 * RL4 + LAT_W * RL4;
      Raw *const to = table + (f0 + j) * RL4;
      bool differs = false;
      for (int64_t v0 = 0; v0 < RL4; v0 += kSyncU * 64) {
        float4 a[kSyncU];
        Raw b[kSyncU];
#pragma unroll
        for (int u = 0; u < kSyncU; u++) {
          const int64_t v = v0 + u * 64 + lane;
          a[u] = v < RL4 ? load_nt(from + v) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
#pragma unroll
        for (int u = 0; u < kSyncU; u++) {
          const int64_t v = v0 + u * 64 + lane;
          b[u] = v < RL4 ? load_nt(to + v) : Raw{};
        }
#pragma unroll
        for (int u = 0; u < kSyncU; u++) {
          const int64_t v = v0 + u * 64 + lane;
          const Raw want = sync_target(a[u], b[u]);
          const unsigned d = v < RL4 ? sync_differ(want, b[u]) : 0u;
          if (d != 0u) to[v] = want;
          n_lat += d;
          differs = differs || d != 0u;
        }
      }
      if (__ballot(differs) != 0ull) word |= 1ull << j;
    }
    if (lane == 0) {
      bitmap[wi] = word;
      n_moved += static_cast<unsigned>(__popcll(word));
    }
  }
  const unsigned part[3] = {n_moved, n_lin, n_lat};  // SY_MOVED, SY_LIN, SY_LAT
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const unsigned long long sum = serve_wave_sum(part[k]);
    if (lane == 0 && sum != 0ull)
      __hip_atomic_fetch_add(counters + k * kPackLine, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ids[j] <-> dense[j][row_len] in the table's own elements (T: 4 bytes for fp32, 2 for fp16), no conversion.
// An id outside [0, n_feats) reads as zero bits and ignores writes.
template <typename T>
__global__ void serve_rows_raw_kernel(ModelDev m, void *dense_raw, const int *ids, int64_t nf, int to_dense) {
  const int64_t RL = m.row_len, total = nf * RL;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  T *const table = reinterpret_cast<T *>(m.lat), *const dense = static_cast<T *>(dense_raw);
  for (int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; idx < total; idx += stride) {
    const int64_t j = idx / RL;
    const int i = ids[j];
    const bool in = i >= 0 && i < m.n_feats;
    const int64_t at = static_cast<int64_t>(i) * RL + (idx - j * RL);
    if (to_dense) dense[idx] = in ? table[at] : static_cast<T>(0);
    else if (in) table[at] = dense[idx];
  }
}

}  // namespace ftrl_dev
