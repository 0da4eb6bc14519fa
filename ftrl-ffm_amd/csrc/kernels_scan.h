// kernels_scan.h -- which features no longer hold what ffm_engine_create gave them
// (ffm_engine_changed_features, the list behind a sparse checkpoint).
//
// Feature i is CHANGED when any 32-bit pattern of its stored state -- lin_w[i], lin_n[i], lin_z[i] and
// its latent record n | z | w -- differs from the create-time pattern: zero bits for every n and z, and
// for w the draw init_weights_kernel stored (ftrl_rng::init_weight at the same logical index; zero bits
// on a FFM_FLAG_SKIP_INIT engine).  Patterns, not values: -0.0f in z is changed, a NaN is changed, a w
// that equals its draw is not.  (n, z) alone would not do: the lazy refresh overwrites w with
// W(0, 0) = 0 for a touched slot whose gradient was exactly zero.
//
// Shape: one wave owns one 64-bit word of the bitmap = 64 consecutive features.  No atomics, no LDS, no
// barriers; the word is built in a (wave-uniform) register and stored once by lane 0 with a vector store.
//   1. lane = feature: the linear triple, coalesced, and its own draw -- one ballot.
//   2. per feature the linear triple has not decided: the lanes stream the record's n and z rows (one
//      contiguous span) as 16-byte non-temporal loads, all of a lane's loads issued before the first OR,
//      OR the patterns, one ballot.  (row_len % 4 != 0: records are not 16-byte aligned, scalar loads.)
//   3. only when n and z are all zero: the w row against the draws, 64 elements at a time, leaving at the
//      first chunk that differs.  A draw is ~150 fp64 operations, so steps 1 and 2 deciding first is what
//      makes a trained or filled model cheap; a fresh model pays the draw for every element.
// Whole-model engines only (n_shards == 1): records are full-length and contiguous at
// m.lat + feat * 3 * row_len, and logical index == stored index.  64-bit element offsets throughout.
#pragma once
#include "engine_types.h"
#include "init_rng.h"

namespace ftrl_dev {

constexpr int kScanThreads = 256;
constexpr int kScanWaves = kScanThreads / 64;

// Words [word0, word0 + n_words) of the bitmap go to bitmap[0 .. n_words); bits past n_feats are zero.
// VEC4: row_len % 4 == 0.  SKIP_INIT: the create-time w is zero bits (then w is one span with n and z).
template <bool VEC4, bool SKIP_INIT>
__global__ __launch_bounds__(kScanThreads) void changed_scan_kernel(ModelDev m, float mean, float stddev,
                                                                    uint64_t seed, int64_t word0, int64_t n_words,
                                                                    unsigned long long *bitmap) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int64_t wi = static_cast<int64_t>(blockIdx.x) * kScanWaves + wv;
  if (wi >= n_words) return;  // (the whole wave)
  const int64_t f0 = (word0 + wi) * 64;
  const int64_t fl = f0 + lane;
  bool lin_changed = false;
  if (fl < m.n_feats) {
    const unsigned bw = __float_as_uint(m.lin_w[fl]), bn = __float_as_uint(m.lin_n[fl]), bz = __float_as_uint(m.lin_z[fl]);
    const unsigned init = SKIP_INIT ? 0u : __float_as_uint(ftrl_rng::init_weight(seed, 0, static_cast<uint64_t>(fl), mean, stddev));
    lin_changed = (bn | bz | (bw ^ init)) != 0u;
  }
  unsigned long long word = __ballot(lin_changed);
  const int64_t RL = m.row_len;
  if (RL > 0) {
    const int nf = static_cast<int>(m.n_feats - f0 < 64 ? m.n_feats - f0 : 64);
    const int64_t span = (SKIP_INIT ? 3 : 2) * RL;  // floats streamed for the zero test
    for (int j = 0; j < nf; j++) {
      if ((word >> j) & 1ull) continue;  // the linear triple has decided
      const float *rec = m.lat + (f0 + j) * 3 * RL;
      unsigned acc = 0u;
      if (VEC4) {
        const float4 *rec4 = reinterpret_cast<const float4 *>(rec);
        const int64_t nv = span / 4;
        for (int64_t v0 = 0; v0 < nv; v0 += 4 * 64) {
          float4 a[4];
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const int64_t v = v0 + u * 64 + lane;
            a[u] = v < nv ? load_nt(rec4 + v) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
          }
#pragma unroll
          for (int u = 0; u < 4; u++)
            acc |= __float_as_uint(a[u].x) | __float_as_uint(a[u].y) | __float_as_uint(a[u].z) | __float_as_uint(a[u].w);
        }
      } else {
        for (int64_t e0 = 0; e0 < span; e0 += 4 * 64) {
          float a[4];
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const int64_t e = e0 + u * 64 + lane;
            a[u] = e < span ? __builtin_nontemporal_load(rec + e) : 0.0f;
          }
#pragma unroll
          for (int u = 0; u < 4; u++) acc |= __float_as_uint(a[u]);
        }
      }
      if (__ballot(acc != 0u) != 0ull) { word |= 1ull << j; continue; }
      if (!SKIP_INIT) {
        const float *w = rec + LAT_W * RL;
        const uint64_t base = static_cast<uint64_t>(f0 + j) * static_cast<uint64_t>(RL);  // init_weights_kernel's index
        for (int64_t e0 = 0; e0 < RL; e0 += 64) {
          const int64_t e = e0 + lane;
          bool differs = false;
          if (e < RL)
            differs = __float_as_uint(__builtin_nontemporal_load(w + e)) !=
                      __float_as_uint(ftrl_rng::init_weight(seed, 1, base + static_cast<uint64_t>(e), mean, stddev));
          if (__ballot(differs) != 0ull) { word |= 1ull << j; break; }
        }
      }
    }
  }
  if (lane == 0) bitmap[wi] = word;
}

}  // namespace ftrl_dev
