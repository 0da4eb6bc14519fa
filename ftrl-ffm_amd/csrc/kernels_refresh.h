// kernels_refresh.h -- every stored weight from its accumulators (ffm_engine_refresh_weights).
//
// Training refreshes w = W(n, z) lazily, for what a block touches, BEFORE the block's update, and prediction
// reads the stored w only: after a run every stored weight is one update behind its (n, z).  This pass
// closes the gap outside the training path: one streaming sweep over everything the engine STORES -- the
// bias triple, lin_n / lin_z / lin_w [n_feats] and the n_records latent records n | z | w of row_len floats
// each.  It walks stored records by position, never by feature id, so one kernel serves a whole-model
// engine and a shard (compact or full-length): padding slots of a compact record, slots a full-length
// shard does not own and linear entries of another shard's fields have n = z = 0 and are dead below.
//
// Rule per element:
//   live    = (bits(n) | bits(z)) != 0        (patterns: -0.0f and NaN are live)
//   dead    : w is not counted and keeps its bits
//   live linear / bias : w_new = ftrl_weight(h, n, z)
//   live latent        : w_new = latent_weight(h, n, z, w_old)   (FFM_FLAG_LEARN: n not > 0 keeps w_old)
//   nonzero = live && !(w_new == 0.0f)        (NaN counts, -0.0f does not)
//   moved   = live && bits(w_new) != bits(w_old)
// (n, z) are never written.  The arithmetic is ftrl_math.h's ftrl_weight_n<4> / latent_weight4, unchanged:
// the bits are those the row kernel's lazy refresh would store for the same (n, z).
//
// Shape: bandwidth-bound by construction -- 12 bytes read per stored element, 4 written where a lane's
// group of four moved.  A persistent grid (sized by the caller from the CU count) strides over a flat
// index space; every lane issues all loads of a turn (2 x {n, z, w} float4 = 96 bytes, non-temporal)
// before the first use.  row_len % 4 != 0: records are not 16-byte aligned, and the lanes take four
// scalar elements a turn instead (VEC4 = false); the linear arrays, 0.2 % of the headline model's bytes,
// always go that way, with the bias as element n_feats.  A lane's position in (record, offset) form is
// advanced by additions: one division per lane and launch.
//
// ftrl_math.h's helpers vote across the wave (__all): every turn's trip count is uniform over the whole
// grid, lanes past the end compute on zeros with their wave and only skip the store and the counts; no
// early return, no divergent call.  A store rewrites a whole group of four: a dead or unmoved element
// beside a moved one gets the bits it was loaded with (nothing else runs on the model during the call).
//
// Counters: six unsigned 64-bit integers, {lin_live, lin_nonzero, lin_moved, lat_live, lat_nonzero,
// lat_moved}; per lane in registers, summed across the wave, one integer atomic per counter and wave at
// the end (none when the wave's sum is zero).  No float atomics, no LDS, no barriers.  64-bit element
// offsets throughout.
#pragma once
#include "engine_types.h"

namespace ftrl_dev {

constexpr int kRefreshThreads = 256;
enum { RC_LIN_LIVE = 0, RC_LIN_NONZERO, RC_LIN_MOVED, RC_LAT_LIVE, RC_LAT_NONZERO, RC_LAT_MOVED, RC_COUNT };

// Per-lane counts.  32 bits: a lane sees (elements / threads of the grid) of them, and the grid has at
// least 64 threads -- 2^38 stored elements would be needed to wrap, a terabyte of model.
struct RefreshCount { unsigned live, nonzero, moved; };

// One group of four: the new weights (LATENT: with the learning variant's exception), counted for the
// components `valid` admits (bit c = component c lies inside the model).  Returns true when the group
// has to be stored.  Called by every lane of the wave together.
template <bool LATENT>
__device__ __forceinline__ bool refresh_group(const Hyper &h, float4 n, float4 z, float4 w_old, unsigned valid,
                                              float4 &w_new, RefreshCount &cnt) {
  const float4 w = LATENT ? latent_weight4(h, n, z, w_old) : ftrl_weight4(h, n, z);
  const float nn[4] = {n.x, n.y, n.z, n.w}, zz[4] = {z.x, z.y, z.z, z.w};
  const float wo[4] = {w_old.x, w_old.y, w_old.z, w_old.w}, wc[4] = {w.x, w.y, w.z, w.w};
  float out[4];
  bool any_moved = false;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const bool live = ((valid >> c) & 1u) && (__float_as_uint(nn[c]) | __float_as_uint(zz[c])) != 0u;
    out[c] = live ? wc[c] : wo[c];
    const bool moved = live && __float_as_uint(wc[c]) != __float_as_uint(wo[c]);
    cnt.live += live ? 1u : 0u;
    cnt.nonzero += (live && !(wc[c] == 0.0f)) ? 1u : 0u;
    cnt.moved += moved ? 1u : 0u;
    any_moved = any_moved || moved;
  }
  w_new = make_float4(out[0], out[1], out[2], out[3]);
  return any_moved;
}

__device__ __forceinline__ unsigned long long refresh_wave_sum(unsigned v) {
  unsigned long long s = v;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  return s;
}

template <bool VEC4>
__global__ __launch_bounds__(kRefreshThreads) void refresh_weights_kernel(ModelDev m, int64_t n_records,
                                                                          unsigned long long *counters) {
  const Hyper h = m.h;
  const int64_t T = static_cast<int64_t>(gridDim.x) * kRefreshThreads;  // lanes of the grid
  const int64_t g = static_cast<int64_t>(blockIdx.x) * kRefreshThreads + threadIdx.x;
  RefreshCount lin{0u, 0u, 0u}, lat{0u, 0u, 0u};

  // ---- linear part: element i < n_feats is (lin_n[i], lin_z[i], lin_w[i]), element n_feats the bias ----
  {
    const int64_t total = static_cast<int64_t>(m.n_feats) + 1;
    for (int64_t i0 = 0; i0 < total; i0 += 4 * T) {  // (uniform over the grid)
      float nn[4], zz[4], ww[4];
      float *pw[4];
      unsigned valid = 0u;
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int64_t i = i0 + u * T + g;
        const bool in = i < total, bias = i == total - 1;
        const float *pn = bias ? m.bias3 + 1 : m.lin_n + i, *pz = bias ? m.bias3 + 2 : m.lin_z + i;
        pw[u] = bias ? m.bias3 : m.lin_w + i;
        nn[u] = in ? __builtin_nontemporal_load(pn) : 0.0f;
        zz[u] = in ? __builtin_nontemporal_load(pz) : 0.0f;
        ww[u] = in ? __builtin_nontemporal_load(pw[u]) : 0.0f;
        valid |= in ? 1u << u : 0u;
      }
      float4 wn;
      refresh_group<false>(h, make_float4(nn[0], nn[1], nn[2], nn[3]), make_float4(zz[0], zz[1], zz[2], zz[3]),
                           make_float4(ww[0], ww[1], ww[2], ww[3]), valid, wn, lin);
      const float wv[4] = {wn.x, wn.y, wn.z, wn.w};
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (((valid >> u) & 1u) && __float_as_uint(wv[u]) != __float_as_uint(ww[u])) __builtin_nontemporal_store(wv[u], pw[u]);
    }
  }

  // ---- latent part: records [0, n_records) of n | z | w, row_len floats each ----
  const int64_t RL = m.row_len;
  if (RL > 0 && n_records > 0) {  // (uniform)
    if (VEC4) {
      // item = one float4 of a record's row: (record r, vector v < RL4); two items a turn, T apart
      constexpr int U = 2;
      const int64_t RL4 = RL / 4, total = n_records * RL4, step = U * T;
      const int64_t dq = step / RL4, dr = step % RL4;  // (uniform: one scalar division)
      float4 *const lat4 = reinterpret_cast<float4 *>(m.lat);
      int64_t r[U], v[U], i[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        i[u] = g + u * T;
        r[u] = i[u] / RL4;
        v[u] = i[u] - r[u] * RL4;
      }
      for (int64_t i0 = 0; i0 < total; i0 += step) {  // (uniform over the grid)
        float4 n4[U], z4[U], w4[U];
        float4 *pw[U];
        bool in[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
          in[u] = i[u] < total;
          float4 *pn = lat4 + r[u] * 3 * RL4 + v[u];
          pw[u] = pn + 2 * RL4;
          const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
          n4[u] = in[u] ? load_nt(pn) : zero;
          z4[u] = in[u] ? load_nt(pn + RL4) : zero;
          w4[u] = in[u] ? load_nt(pw[u]) : zero;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
          float4 wn;
          const bool st = refresh_group<true>(h, n4[u], z4[u], w4[u], in[u] ? 0xfu : 0u, wn, lat);
          if (st) store_nt(pw[u], wn);
          i[u] += step;
          r[u] += dq;
          v[u] += dr;
          if (v[u] >= RL4) { v[u] -= RL4; r[u] += 1; }
        }
      }
    } else {
      // item = one element of a record's row: (record r, element c < RL); four items a turn, T apart
      const int64_t total = n_records * RL, step = 4 * T;
      const int64_t dq = step / RL, dr = step % RL;
      int64_t r[4], c[4], i[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        i[u] = g + u * T;
        r[u] = i[u] / RL;
        c[u] = i[u] - r[u] * RL;
      }
      for (int64_t i0 = 0; i0 < total; i0 += step) {  // (uniform over the grid)
        float nn[4], zz[4], ww[4];
        float *pw[4];
        unsigned valid = 0u;
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const bool in = i[u] < total;
          const float *pn = m.lat + r[u] * 3 * RL + c[u];
          pw[u] = const_cast<float *>(pn) + 2 * RL;
          nn[u] = in ? __builtin_nontemporal_load(pn) : 0.0f;
          zz[u] = in ? __builtin_nontemporal_load(pn + RL) : 0.0f;
          ww[u] = in ? __builtin_nontemporal_load(pw[u]) : 0.0f;
          valid |= in ? 1u << u : 0u;
        }
        float4 wn;
        refresh_group<true>(h, make_float4(nn[0], nn[1], nn[2], nn[3]), make_float4(zz[0], zz[1], zz[2], zz[3]),
                            make_float4(ww[0], ww[1], ww[2], ww[3]), valid, wn, lat);
        const float wv[4] = {wn.x, wn.y, wn.z, wn.w};
#pragma unroll
        for (int u = 0; u < 4; u++) {
          if (((valid >> u) & 1u) && __float_as_uint(wv[u]) != __float_as_uint(ww[u])) __builtin_nontemporal_store(wv[u], pw[u]);
          i[u] += step;
          r[u] += dq;
          c[u] += dr;
          if (c[u] >= RL) { c[u] -= RL; r[u] += 1; }
        }
      }
    }
  }

  // ---- one atomic per counter and wave ----
  const unsigned part[RC_COUNT] = {lin.live, lin.nonzero, lin.moved, lat.live, lat.nonzero, lat.moved};
#pragma unroll
  for (int k = 0; k < RC_COUNT; k++) {
    const unsigned long long s = refresh_wave_sum(part[k]);
    if ((threadIdx.x & 63) == 0 && s != 0ull)
      __hip_atomic_fetch_add(counters + k, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace ftrl_dev
