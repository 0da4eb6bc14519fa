// kernels_pruned.h -- a PRUNED serving table (include/ffm_engine.h "Pruned serving tables"): the packed table of a
// serving engine with the slots of dropped pairs gone from memory, for models whose ids lie in per-field ranges.
//
// keep[n_fields] is a pair mask (kernels_mask.h), field_start[n_fields + 1] the fields' id ranges.  A feature i of
// field f owns P[f] = popcount(keep[f]) consecutive slots of n_factors elements from slot
//   first(i) = base[f] + (i - field_start[f]) * P[f],   base = prefix sum of (field_start[f + 1] - field_start[f]) * P[f]
// and its slot towards partner g sits at rank(f, g) = popcount(keep[f] & ((1 << g) - 1)) behind it.  The table has
// fewer than 2^32 slots (create checked), so a slot number is one 32-bit word; element offsets are 64-bit.
//
//   ffm_row_pruned_kernel     ffm_row_mask_kernel on this table: the same walk, queue, gathers and ordered sum of the
//                             kept pairs -- WavePairCursor, wave_pair_term and wave_ordered_sum of kernels_wave.h as
//                             they are, wave_stage_entries with the range test added -- and its own addressing.  While
//                             an entry is staged its lane resolves the field's range ONCE: whether the id lies in it
//                             (otherwise the entry is erased whole, as an id >= n_feats is) and first(i), which
//                             travels in the staged int4's fourth word.  A pair's two gather addresses are then
//                             (first(a) + rank(fa, fb)) * n_factors and (first(b) + rank(fb, fa)) * n_factors: per
//                             address one mask word from LDS, a shift-and-mask and a popcount.  Nothing in global
//                             memory is read per pair but the slots themselves.
//                             The queue stays at (pa, pb) in 16 bits: carrying the two ranks would double it and
//                             move two LDS reads and popcounts from the gather step (kept pairs only) to the walk
//                             (every candidate), and the gather step has the VGPRs for them inside the six waves
//                             per SIMD of FFM_PRED_OCC.
//   pruned_init_kernel        the create-time contents: a training engine's draw at the element's full-length index
//   pruned_rows_copy_kernel   full-length fp32 rows in the staging buffer <-> the table, by id list or by range
//   serve_pack_pruned_kernel  a training engine's stored bias, lin_w and the KEPT slots of w into the table, counted
//
// LDS per wave of the row kernel: the staged entries and the batch of terms (pred_lds_bytes), the queue (640 bytes),
// the 64 mask words (512), and field_start[] and base[] of 66 words each (528), all staged once per wave with no
// barrier: 4752 bytes at 128 entries, 18.6 KB per workgroup -- six workgroups of four waves per CU (the kernel's six
// waves per SIMD) are 111 KB of the CU's 160 KB, so LDS is not what limits occupancy.
#pragma once
#include "engine_types.h"
#include "init_rng.h"
#include "kernels_mask.h"
#include "kernels_serve.h"
#include "kernels_wave.h"

namespace ftrl_dev {

struct PrunedDev {
  const unsigned long long *keep;  // [kMaskFields] the mask words, zero from n_fields on
  const int *field_start;          // [n_fields + 1]
  const unsigned *base;            // [n_fields + 1] first slot of a field's first feature; [n_fields]: the table's slots
};

constexpr int kPrunedTab = kMaskFields + 2;  // words of field_start[] / base[] in a wave's LDS (n_fields + 1 used)
constexpr int kPrunedLdsWords = kMaskLdsWords + 2 * kPrunedTab;

__host__ __device__ inline size_t pruned_lds_bytes(int lds_cap) {
  return static_cast<size_t>(kPredRows) * (static_cast<size_t>(lds_cap) * 16 + (kPredTerms + kPrunedLdsWords) * 4);
}

__device__ __forceinline__ int pruned_rank(unsigned long long keep_f, int g) { return __popcll(keep_f & ((1ull << g) - 1ull)); }

// The field whose id range holds `feat` (0 <= feat < n_feats): the last f with start[f] <= feat.
__device__ __forceinline__ int pruned_field_of(const int *start, int n_fields, int64_t feat) {
  int lo = 0, hi = n_fields;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (start[mid] <= feat) lo = mid; else hi = mid;
  }
  return lo;
}

// wave_stage_entries (kernels_wave.h) for this table: the same compaction in row order and the same strictly
// sequential linear prefix, but an entry survives only if its id also lies in its field's range -- its lane has the
// range's two words from LDS anyway, for the feature's first slot, which goes into the staged entry's fourth word.
// (Its own loop, not a hook in wave_stage_entries: the other wave kernels' code is not to move.)
__device__ __forceinline__ void pruned_stage_entries(const ModelDev &m, const Rows &rows, int b, int nnz, int lane, const int *FS,
                                                     const unsigned *B, const unsigned long long *K, int4 *E, float &result,
                                                     int &nv) {
  for (int base = 0; base < nnz; base += 64) {
    const int p = base + lane;
    int i = 0, f = 0;
    unsigned first = 0u;
    float x = 0.0f, lw = 0.0f;
    bool valid = false;
    if (p < nnz) {
      i = rows.feat[b + p];
      f = rows.field[b + p];
      x = rows.val[b + p];
      valid = i >= 0 && i < m.n_feats && f >= 0 && f < m.n_fields;
    }
    if (valid) {
      const int lo = FS[f];
      valid = i >= lo && i < FS[f + 1];
      // (i - lo) * P is below the field's slots, so below 2^32
      first = B[f] + static_cast<unsigned>(i - lo) * static_cast<unsigned>(__popcll(K[f]));
    }
    if (valid) lw = m.lin_w[i];
    const unsigned long long mask = __ballot(valid);
    if (valid) E[nv + __popcll(mask & ((1ull << lane) - 1ull))] = make_int4(i, f, __float_as_int(x), static_cast<int>(first));
    nv += __popcll(mask);
    // x + -0.0f == x bit for bit: idle lanes and erased entries add nothing
    const float run = wave_sequential_prefix(result, valid ? lw * x : -0.0f);
    result = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(run), 63));
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
}

template <int FMT, int LPP, int VPL, int U>
__global__ __launch_bounds__(64 * kPredRows) FFM_PRED_OCC void ffm_row_pruned_kernel(ModelDev m, Rows rows, Scratch s,
                                                                       int max_row_nnz, int lds_cap, float *out,
                                                                       int output_prob, PrunedDev pd) {
  static_assert(FMT == SERVE_F32 || FMT == SERVE_F16, "a packed table of w alone");
  constexpr int PPS = wave_pairs_per_step<LPP, U>();
  using Raw = typename WaveTable<FMT>::Raw;
  static_assert(kPredLdsCap <= 256, "a queued pair is two bytes");
  static_assert((kPredTerms * 4 + kMaskQueue * 2) % 8 == 0, "the mask words are 8-byte aligned");
  static_assert((kPredTerms + kPrunedLdsWords) % 4 == 0, "the next wave's entries are 16-byte aligned");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = wave_uniform(blockIdx.x * kPredRows + wv);
  if (r >= rows.n_rows) return;
  const WaveLds lds = wave_lds(smem, wv, lds_cap, kPredTerms + kPrunedLdsWords);
  int4 *const E = lds.E;
  unsigned short *const Q = reinterpret_cast<unsigned short *>(lds.terms + kPredTerms);  // [kMaskQueue]
  unsigned long long *const K = reinterpret_cast<unsigned long long *>(Q + kMaskQueue);  // [kMaskFields]
  int *const FS = reinterpret_cast<int *>(K + kMaskFields);                               // [kPrunedTab]
  unsigned *const B = reinterpret_cast<unsigned *>(FS + kPrunedTab);                      // [kPrunedTab]
  const int b = wave_uniform(rows.row_ptr[r]);
  const int nnz = wave_uniform(rows.row_ptr[r + 1]) - b;
  if (nnz > max_row_nnz || nnz > lds_cap) {  // flagged, NaN outputs (no launch behind this one takes the row)
    if (lane == 0) {
      atomicOr(s.err, ERR_ROW_TOO_LONG);
      const float nan = __int_as_float(0x7fc00000);
      s.loss[r] = static_cast<double>(nan);
      if (out) out[r] = nan;
    }
    return;
  }
  const Raw *const w = reinterpret_cast<const Raw *>(m.lat);
  const int k4 = m.n_factors >> 2;

  K[lane] = lane < m.n_fields ? pd.keep[lane] : 0ull;  // (n_fields <= kMaskFields: create checked)
  for (int t = lane; t <= m.n_fields; t += 64) {
    FS[t] = pd.field_start[t];
    B[t] = pd.base[t];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  float result = m.bias3[0];
  int nv = 0;
  pruned_stage_entries(m, rows, b, nnz, lane, FS, B, K, E, result, nv);

  const int n_pairs = nv * (nv - 1) / 2;
  const int g = lane / LPP, c = lane - g * LPP;
  WavePairCursor walk;  // this lane's candidate of the coming walk step: number cand + lane
  walk.start(lane, n_pairs, nv);
  int cand = 0;  // candidates walked so far
  int qn = 0;    // pairs in the queue
  while (cand < n_pairs || qn > 0) {
    // ---- the walk: until a batch is queued or the candidates are through
    while (qn < kPredTerms && cand < n_pairs) {
      const bool live = cand + lane < n_pairs;
      bool kept = false;
      if (live) {
        const int fa = E[walk.pa].y, fb = E[walk.pb].y;
        kept = (K[fa] >> fb) & 1ull;
      }
      const unsigned long long hit = __ballot(kept);
      if (kept) Q[qn + __popcll(hit & ((1ull << lane) - 1ull))] = static_cast<unsigned short>(walk.pa | (walk.pb << 8));
      qn += __popcll(hit);
      if (cand + lane + 64 < n_pairs) walk.advance(64, nv);
      cand += 64;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    const int cnt = min(qn, kPredTerms);
    // ---- the gathers of the batch: Q[0 .. cnt) in pair order.  A kept pair's two slots exist (both ids lie in
    // their fields' ranges and the bit is set both ways); an idle group reads slot 0, which exists whenever any
    // pair is kept (cnt > 0), and its term goes nowhere.
    for (int st = 0; st * PPS < cnt; st += U) {
      Raw x[U][VPL], y[U][VPL];
      float xa[U], xb[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int t = (st + u) * PPS + g;  // (< kPredTerms: inside the queue whatever cnt is)
        ok[u] = t < cnt;
        const int qe = ok[u] ? Q[t] : 0;
        const int4 ea = E[qe & 0xff], eb = E[qe >> 8];
        xa[u] = __int_as_float(ea.z);
        xb[u] = __int_as_float(eb.z);
        const unsigned sa = ok[u] ? static_cast<unsigned>(ea.w) + pruned_rank(K[ea.y], eb.y) : 0u;
        const unsigned sb = ok[u] ? static_cast<unsigned>(eb.w) + pruned_rank(K[eb.y], ea.y) : 0u;
        const Raw *va = w + static_cast<int64_t>(sa) * k4 + c * VPL, *vb = w + static_cast<int64_t>(sb) * k4 + c * VPL;
#pragma unroll
        for (int v = 0; v < VPL; v++) { x[u][v] = va[v]; y[u][v] = vb[v]; }
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        const float term = wave_pair_term<LPP, VPL>(x[u], y[u], c, xa[u], xb[u]);
        if (c == LPP - 1 && ok[u]) lds.terms[(st + u) * PPS + g] = term;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    result = wave_ordered_sum(result, lds.terms, cnt, lane);
    // ---- what the walk queued beyond the batch (fewer than 64 pairs) to the queue's head
    const int rest = qn - cnt;
    unsigned short moved = 0;
    if (lane < rest) moved = Q[cnt + lane];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    if (lane < rest) Q[lane] = moved;
    qn = rest;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  }

  if (lane == 0) {
    out[r] = output_prob ? sigmoid_ref(result) : result;
    if (rows.label) s.loss[r] = logloss_ref(rows.label[r], result);
  }
}

// ---- the streaming kernels ------------------------------------------------------------------------------------

constexpr int kPrunedThreads = 256;

// sel[f][r] = the partner field of rank r in keep[f], for a workgroup of kPrunedThreads: 4 KB of LDS.
__device__ __forceinline__ void pruned_stage_sel(const PrunedDev &pd, int n_fields, unsigned char (*sel)[kMaskFields]) {
  for (int t = threadIdx.x; t < n_fields * kMaskFields; t += kPrunedThreads) {
    const int f = t / kMaskFields, gg = t - f * kMaskFields;
    const unsigned long long kf = pd.keep[f];
    if ((kf >> gg) & 1ull) sel[f][pruned_rank(kf, gg)] = static_cast<unsigned char>(gg);
  }
  __syncthreads();
}

// Create-time contents: every stored element is the draw of its full-length index, in the format.  One thread per
// stored element, grid-stride: the work is the pruned table's, not the full one's.
__global__ __launch_bounds__(kPrunedThreads) void pruned_init_kernel(ModelDev m, PrunedDev pd, float mean, float stddev, uint64_t seed) {
  __shared__ unsigned char sel[kMaskFields][kMaskFields];
  pruned_stage_sel(pd, m.n_fields, sel);
  const int k = m.n_factors;
  const int64_t RL = static_cast<int64_t>(m.n_fields) * k;
  const int64_t n_el = static_cast<int64_t>(pd.base[m.n_fields]) * k;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kPrunedThreads;
  const int64_t t0 = static_cast<int64_t>(blockIdx.x) * kPrunedThreads + threadIdx.x;
  for (int64_t idx = t0; idx < n_el; idx += stride) {
    const unsigned slot = static_cast<unsigned>(idx / k);
    const int j = static_cast<int>(idx - static_cast<int64_t>(slot) * k);
    int lo = 0, hi = m.n_fields;  // the last field with base[f] <= slot: base[f + 1] > slot, so P[f] > 0
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (pd.base[mid] <= slot) lo = mid; else hi = mid;
    }
    const unsigned P = static_cast<unsigned>(__popcll(pd.keep[lo])), local = slot - pd.base[lo];
    const int64_t feat = pd.field_start[lo] + static_cast<int64_t>(local / P);
    const int gg = sel[lo][local % P];
    serve_store_elem(m, idx, ftrl_rng::init_weight(seed, 1, feat * RL + static_cast<int64_t>(gg) * k + j, mean, stddev));
  }
  for (int64_t i = t0; i < m.n_feats; i += stride) m.lin_w[i] = ftrl_rng::init_weight(seed, 0, i, mean, stddev);
}

// dense[nf][n_fields * n_factors] fp32 <-> the table: row j is feature ids[j], or feat0 + j when ids is null.
// to_dense: a dropped slot (and a feature outside [0, n_feats)) reads +0.0f; otherwise writes to them are ignored.
__global__ __launch_bounds__(kPrunedThreads) void pruned_rows_copy_kernel(ModelDev m, PrunedDev pd, float *dense, const int *ids,
                                                                          int64_t feat0, int64_t nf, int to_dense) {
  const int k = m.n_factors;
  const int64_t RL = static_cast<int64_t>(m.n_fields) * k, total = nf * RL;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kPrunedThreads;
  for (int64_t idx = static_cast<int64_t>(blockIdx.x) * kPrunedThreads + threadIdx.x; idx < total; idx += stride) {
    const int64_t j = idx / RL;
    const int e = static_cast<int>(idx - j * RL);
    const int64_t i = ids ? ids[j] : feat0 + j;
    int64_t at = -1;
    if (i >= 0 && i < m.n_feats) {
      const int f = pruned_field_of(pd.field_start, m.n_fields, i), gg = e / k;
      const unsigned long long kf = pd.keep[f];
      if ((kf >> gg) & 1ull) {
        const unsigned first = pd.base[f] + static_cast<unsigned>(i - pd.field_start[f]) * static_cast<unsigned>(__popcll(kf));
        at = static_cast<int64_t>(first + pruned_rank(kf, gg)) * k + (e - gg * k);
      }
    }
    if (to_dense) dense[idx] = at >= 0 ? serve_load_elem(m, at) : 0.0f;
    else if (at >= 0) serve_store_elem(m, at, dense[idx]);
  }
}

// ffm_engine_pack_weights into a pruned table: G lanes per feature (16 or 64, the host's choice by the longest
// pruned row), grid-stride over the features.  A lane's item is 16 bytes of the feature's pruned row: VPI vectors of
// four factors -- one of fp32; two of fp16 where a slot is 16 bytes or more (n_factors >= 8), else one and 8 bytes.
// Each vector is read from the kept slot of src's record it belongs to (non-temporal: the record streams through
// once) and nothing else of the record is touched.  The counters are serve_pack_kernel's.
template <int FMT, int VPI, int G>
__global__ __launch_bounds__(kPrunedThreads) void serve_pack_pruned_kernel(ModelDev src, ModelDev dst, PrunedDev pd,
                                                                           unsigned long long *counters) {
  static_assert(FMT == SERVE_F32 ? VPI == 1 : (FMT == SERVE_F16 && (VPI == 1 || VPI == 2)), "16 bytes per lane at the most");
  __shared__ unsigned char sel[kMaskFields][kMaskFields];
  pruned_stage_sel(pd, dst.n_fields, sel);
  const int64_t T = static_cast<int64_t>(gridDim.x) * kPrunedThreads;
  const int64_t t0 = static_cast<int64_t>(blockIdx.x) * kPrunedThreads + threadIdx.x;
  for (int64_t i = t0; i < src.n_feats; i += T) dst.lin_w[i] = __builtin_nontemporal_load(src.lin_w + i);
  if (t0 == 0) dst.bias3[0] = src.bias3[0];
  const int k4 = src.n_factors >> 2;
  const int64_t RL4 = src.row_len / 4;  // (src stores full-length records: pack_weights checked)
  const float4 *const rec = reinterpret_cast<const float4 *>(src.lat);
  const int l = threadIdx.x % G;
  unsigned part[PK_COUNT] = {0u, 0u, 0u, 0u};
  for (int64_t i = t0 / G; i < src.n_feats; i += T / G) {
    const int f = pruned_field_of(pd.field_start, dst.n_fields, i);
    const unsigned long long kf = pd.keep[f];
    const int P = __popcll(kf), PV = P * k4;  // vectors of the feature's pruned row
    const int64_t first4 = static_cast<int64_t>(pd.base[f] + static_cast<unsigned>(i - pd.field_start[f]) * static_cast<unsigned>(P)) * k4;
    const float4 *const wrow = rec + i * 3 * RL4 + LAT_W * RL4;
    for (int v0 = l * VPI; v0 < PV; v0 += G * VPI) {
      float4 wv[VPI];
#pragma unroll
      for (int q = 0; q < VPI; q++) {
        const int v = min(v0 + q, PV - 1), rk = v / k4;
        wv[q] = load_nt(wrow + static_cast<int>(sel[f][rk]) * k4 + (v - rk * k4));
      }
      const int n_v = min(VPI, PV - v0);
      if (FMT == SERVE_F32) {
        store_nt(reinterpret_cast<float4 *>(dst.lat) + first4 + v0, wv[0]);
      } else {
        uint2 h[VPI];
#pragma unroll
        for (int q = 0; q < VPI; q++) {
          h[q] = serve_enc16x4(wv[q]);
          if (q >= n_v) continue;
          const float4 d = serve_dec16x4(h[q]);
          const float ws[4] = {wv[q].x, wv[q].y, wv[q].z, wv[q].w}, ds[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
          for (int cc = 0; cc < 4; cc++) {
            const bool nan = ws[cc] != ws[cc];
            part[PK_INEXACT] += (!nan && __float_as_uint(ds[cc]) != __float_as_uint(ws[cc])) ? 1u : 0u;
            part[PK_TO_INF] += (!nan && !isinf(ws[cc]) && isinf(ds[cc])) ? 1u : 0u;
            part[PK_TO_ZERO] += (!nan && ws[cc] != 0.0f && ds[cc] == 0.0f) ? 1u : 0u;
          }
        }
        uint2 *const to = reinterpret_cast<uint2 *>(dst.lat) + first4 + v0;
        if (VPI == 2 && n_v == 2) *reinterpret_cast<uint4 *>(to) = make_uint4(h[0].x, h[0].y, h[VPI - 1].x, h[VPI - 1].y);
        else to[0] = h[0];
      }
      part[PK_LATENT] += 4u * n_v;
    }
  }
#pragma unroll
  for (int c = 0; c < PK_COUNT; c++) {
    const unsigned long long sum = serve_wave_sum(part[c]);
    if ((threadIdx.x & 63) == 0 && sum != 0ull)
      __hip_atomic_fetch_add(counters + c * kPackLine, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace ftrl_dev
