// kernels_mask.h -- prediction under a pair mask (include/ffm_engine.h "Pair masks"): ffm_row_wave_kernel's masked
// twin, for a training engine's evaluation and a serving engine alike.
//
// keep[n_fields] holds one 64-bit word per field: bit g of keep[f] says that the terms between an entry of field f
// and an entry of field g belong to the prediction.  The masked logit of a row is the row kernel's ordered sum --
// bias, the survivors' linear products, then the pair terms in its pair order (a outer, b inner) -- with the terms
// of dropped pairs LEFT OUT: they are neither gathered nor added.
//
// A row is one wave, built from the pieces of kernels_wave.h as they are.  What is new is a queue between the pair
// walk and the gathers:
//   the walk    one lane per candidate pair, 64 per step (WavePairCursor at a stride of 64): the lane reads the two
//               entries' fields, tests the bit, and the kept (pa, pb) are compacted by ballot and popcount -- in
//               pair order -- behind the queue's tail in the wave's LDS (pa, pb < 128: 16 bits a pair).  The walk
//               stops as soon as the queue holds a batch of kPredTerms.
//   the gathers ffm_row_wave_kernel's U-step loop (LPP lanes per pair, U steps of loads in flight) over the first
//               kPredTerms queued pairs instead of over the cursor; then the ordered sum of exactly those terms.
//               What the walk queued beyond the batch (at most 63 pairs) moves to the queue's head.
// So a row's loads, dots and ordered-sum chunks are those of its kept pairs; what stays per row whatever the mask
// says is the staging, the linear prefix and ceil(n_pairs / 64) walk steps of two LDS reads each.
//
// LDS per wave: the staged entries and the batch of terms (as pred_lds_bytes), the queue of kPredTerms + 64 pairs
// (640 bytes) and the 64 mask words (512 bytes, staged once per wave: no barrier): 4224 bytes at 128 entries,
// 16.5 KB per workgroup -- six workgroups of four waves per CU (the kernel's six waves per SIMD) are 99 KB of the
// CU's 160 KB, so LDS is not what limits occupancy.
//
// A row longer than max_row_nnz or than the entries a wave stages is NaN and flagged on every kind of engine: a
// masked engine has no second launch behind this one.
#pragma once
#include "engine_types.h"
#include "kernels_wave.h"

namespace ftrl_dev {

constexpr int kMaskFields = 64;                                        // n_fields at the most: a word per field
constexpr int kMaskQueue = kPredTerms + 64;                            // pairs the queue holds: a batch and one walk step
constexpr int kMaskLdsWords = kMaskQueue * 2 / 4 + kMaskFields * 2;    // 4-byte words behind a wave's terms: queue, mask

__host__ __device__ inline size_t mask_lds_bytes(int lds_cap) {
  return static_cast<size_t>(kPredRows) * (static_cast<size_t>(lds_cap) * 16 + (kPredTerms + kMaskLdsWords) * 4);
}

// The words of a new mask come as a kernel argument (read when the launch is made: nothing of the caller's has to
// outlive the call) and are stored behind the kernels that still read the previous ones.  One wave.
struct PairMaskWords {
  unsigned long long w[kMaskFields];
};
__global__ __launch_bounds__(kMaskFields) void pair_mask_store_kernel(PairMaskWords k, unsigned long long *dst) {
  dst[threadIdx.x] = k.w[threadIdx.x];
}

template <int FMT, int LPP, int VPL, int U>
__global__ __launch_bounds__(64 * kPredRows) FFM_PRED_OCC void ffm_row_mask_kernel(ModelDev m, Rows rows, Scratch s,
                                                                     int max_row_nnz, int lds_cap, float *out,
                                                                     int output_prob, const unsigned long long *keep) {
  constexpr int PPS = wave_pairs_per_step<LPP, U>();
  using Raw = typename WaveTable<FMT>::Raw;
  static_assert(kPredLdsCap <= 256, "a queued pair is two bytes");
  static_assert((kPredTerms * 4 + kMaskQueue * 2) % 8 == 0, "the mask words are 8-byte aligned");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = wave_uniform(blockIdx.x * kPredRows + wv);
  if (r >= rows.n_rows) return;
  const WaveLds lds = wave_lds(smem, wv, lds_cap, kPredTerms + kMaskLdsWords);
  int4 *const E = lds.E;
  unsigned short *const Q = reinterpret_cast<unsigned short *>(lds.terms + kPredTerms);  // [kMaskQueue]
  unsigned long long *const K = reinterpret_cast<unsigned long long *>(Q + kMaskQueue);  // [kMaskFields]
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
  const WaveTable<FMT> table(m);

  K[lane] = lane < m.n_fields ? keep[lane] : 0ull;  // (n_fields <= kMaskFields: the engine checked)
  float result = m.bias3[0];
  int nv = 0;
  wave_stage_entries(m, rows.feat, rows.field, rows.val, b, nnz, lane, result, nv, [&](int at, int4 en, float) { E[at] = en; });

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
    // ---- the gathers of the batch: Q[0 .. cnt) in pair order (cnt > 0 implies nv >= 2: entries 0 and 1 exist)
    for (int st = 0; st * PPS < cnt; st += U) {
      Raw x[U][VPL], y[U][VPL];
      float xa[U], xb[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int t = (st + u) * PPS + g;  // (< kPredTerms: inside the queue whatever cnt is)
        ok[u] = t < cnt;
        const int qe = ok[u] ? Q[t] : 0x100;
        const int4 ea = E[qe & 0xff], eb = E[qe >> 8];
        xa[u] = __int_as_float(ea.z);
        xb[u] = __int_as_float(eb.z);
        const Raw *va = table.slot(ea.x, eb.y) + c * VPL, *vb = table.slot(eb.x, ea.y) + c * VPL;
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
    // ---- what the walk queued beyond the batch (fewer than 64 pairs) to the queue's head: one read of every
    // lane, then one write
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

}  // namespace ftrl_dev
