// kernels_curve.h -- the pruning curve in one pass (include/ffm_engine.h "Pruning curve"): for every row the n_cuts
// logits "the row without the pair terms whose level is at or above cut c" (c < n_cuts) and "the row itself"
// (c = n_cuts).
//   ffm_curve_wave_kernel   ffm_ablate_wave_kernel's structure (kernels_ablate.h) with another predicate: one wave
//                           per row, the pieces of kernels_wave.h as they are, the gathers and the k-long dots made
//                           once per row.
// The loss sums and the histograms are ablate_loss_sum_kernel and ablate_hist_kernel (kernels_ablate.h), unchanged,
// with gridDim.y = n_cuts + 1.
//
// level[n_fields][n_fields] (16 bits an entry, symmetric, in HBM: 8 KB at 64 fields, so it stays in cache) says
// where on the ladder a field pair stands; variant c leaves out the terms whose pair has level >= cut[c].  No
// linear term is ever left out, so every variant starts from the row's own staged prefix -- bias and linear
// products -- and there is no linear walk.  Lane c keeps variant c's running value in one register and cut[c] in
// another.  The lane that stores a term also stores the term's level into a second per-wave array beside the
// terms; after the batch's ordered sum every lane walks the batch in pair order: two broadcast LDS reads per
// term (the level, the term), one compare and one dependent add, four terms' reads ahead of their four adds.
// Leaving a term out and adding -0.0f in its place are the same bits (x + -0.0f == x), so variant c is what
// ffm_row_mask_kernel returns for the mask "level < cut[c]".
//
// LDS per wave: the staged entries, the batch of terms and the batch of levels (4 bytes each: the compare reads
// them as they are): 4 KB at 128 entries, 16 KB per workgroup -- six workgroups of four waves per CU (the kernel's
// six waves per SIMD) are 96 KB of the CU's 160 KB.
#pragma once
#include "engine_types.h"
#include "kernels_ablate.h"
#include "kernels_wave.h"

namespace ftrl_dev {

constexpr int kCurveCuts = 64;      // cuts at the most: one lane each
constexpr int kCurveFields = 64;    // n_fields at the most, as for the other kinds
constexpr int kCurveLevelMax = 65536;  // a cut at the most: above every level, so it drops nothing

__host__ __device__ inline size_t curve_lds_bytes(int lds_cap) {
  return static_cast<size_t>(kPredRows) * (static_cast<size_t>(lds_cap) * 16 + 2 * kPredTerms * 4);
}

// What a curve is on the device: engine-owned arrays in HBM.
struct CurveDev {
  const unsigned short *level;  // [n_fields][n_fields]
  const int *cut;               // [n_cuts]
  int n_cuts;                   // 1 .. kCurveCuts
};

// FMT: WaveTable's.  out[(n_cuts + 1) * n_rows] variant-major; loss[(n_cuts + 1) * loss_stride], written when labels came.
template <int FMT, int LPP, int VPL, int U>
__global__ __launch_bounds__(64 * kPredRows) FFM_PRED_OCC void ffm_curve_wave_kernel(ModelDev m, Rows rows, int *err,
                                                                       int max_row_nnz, int lds_cap, float *out,
                                                                       double *loss, int loss_stride, int output_prob,
                                                                       CurveDev cv) {
  constexpr int PPS = wave_pairs_per_step<LPP, U>();
  using Raw = typename WaveTable<FMT>::Raw;
  static_assert(kPredTerms % 4 == 0, "the walk's unrolled part reads whole fours");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = wave_uniform(blockIdx.x * kPredRows + wv);
  if (r >= rows.n_rows) return;
  const WaveLds lds = wave_lds(smem, wv, lds_cap, 2 * kPredTerms);
  int4 *const E = lds.E;
  float *const terms = lds.terms;
  int *const lvl = reinterpret_cast<int *>(lds.terms + kPredTerms);  // [kPredTerms] the batch's levels
  const int b = wave_uniform(rows.row_ptr[r]);
  const int nnz = wave_uniform(rows.row_ptr[r + 1]) - b;
  const int F = m.n_fields;      // (<= kCurveFields: the engine checked)
  const int C = cv.n_cuts;       // (<= 64: one lane per variant c < C, lane 0 also variant C)
  const size_t at = static_cast<size_t>(lane) * rows.n_rows + r;  // variant `lane` of this row in out
  const size_t at_loss = static_cast<size_t>(lane) * loss_stride + r;
  const size_t whole = static_cast<size_t>(C) * rows.n_rows + r, whole_loss = static_cast<size_t>(C) * loss_stride + r;
  // beyond the validated capacity or what a wave stages (there is no second launch behind this one): flagged,
  // NaN in every variant
  if (nnz > max_row_nnz || nnz > lds_cap) {
    const float nan = __int_as_float(0x7fc00000);
    if (lane == 0) {
      atomicOr(err, ERR_ROW_TOO_LONG);
      out[whole] = nan;
      if (rows.label) loss[whole_loss] = static_cast<double>(nan);
    }
    if (lane < C) {
      out[at] = nan;
      if (rows.label) loss[at_loss] = static_cast<double>(nan);
    }
    return;
  }
  const WaveTable<FMT> table(m);
  const int my_cut = lane < C ? cv.cut[lane] : kCurveLevelMax;  // (an idle lane drops nothing and writes nothing)

  float result = m.bias3[0];
  int nv = 0;
  wave_stage_entries(m, rows.feat, rows.field, rows.val, b, nnz, lane, result, nv, [&](int at, int4 en, float) { E[at] = en; });
  float acc = result;  // every variant's linear part is the row's own

  // ---- pairs, as the row kernel walks them
  const int n_pairs = nv * (nv - 1) / 2;
  const int g = lane / LPP, c = lane - g * LPP;
  WavePairCursor cur;
  cur.start(g, n_pairs, nv);
  for (int q0 = 0; q0 < n_pairs; q0 += kPredTerms) {
    const int cnt = min(kPredTerms, n_pairs - q0);
    for (int st = 0; st * PPS < cnt; st += U) {
      Raw x[U][VPL], y[U][VPL];
      float xa[U], xb[U];
      int lv[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int q = q0 + (st + u) * PPS + g;
        ok[u] = q < n_pairs;
        const int a = ok[u] ? cur.pa : 0, bb = ok[u] ? cur.pb : (nv > 1 ? 1 : 0);
        const int4 ea = E[a], eb = E[bb];
        xa[u] = __int_as_float(ea.z);
        xb[u] = __int_as_float(eb.z);
        const Raw *va = table.slot(ea.x, eb.y) + c * VPL, *vb = table.slot(eb.x, ea.y) + c * VPL;
#pragma unroll
        for (int v = 0; v < VPL; v++) { x[u][v] = va[v]; y[u][v] = vb[v]; }
        lv[u] = cv.level[ea.y * F + eb.y];  // (survivors' fields: inside the table; a pair's lanes read one address)
        if (q + PPS < n_pairs) cur.advance(PPS, nv);
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        const float term = wave_pair_term<LPP, VPL>(x[u], y[u], c, xa[u], xb[u]);
        if (c == LPP - 1 && ok[u]) {
          terms[(st + u) * PPS + g] = term;
          lvl[(st + u) * PPS + g] = lv[u];
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    result = wave_ordered_sum(result, terms, cnt, lane);
    // ---- the variants' share of the batch: its terms in order, lane c leaving out what stands at or above its cut
    {
      int t = 0;
      for (; t + 4 <= cnt; t += 4) {
        int l[4], tb[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { l[u] = lvl[t + u]; tb[u] = __float_as_int(terms[t + u]); }
        ablate_pin4(l, tb);
#pragma unroll
        for (int u = 0; u < 4; u++) acc = ablate_add(acc, l[u] >= my_cut, tb[u]);
      }
      for (; t < cnt; t++) {
        int l = lvl[t], tb = __float_as_int(terms[t]);
        ablate_pin(l, tb);
        acc = ablate_add(acc, l >= my_cut, tb);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  }

  if (lane == 0) {
    out[whole] = output_prob ? sigmoid_ref(result) : result;
    if (rows.label) loss[whole_loss] = logloss_ref(rows.label[r], result);
  }
  if (lane < C) {
    out[at] = output_prob ? sigmoid_ref(acc) : acc;
    if (rows.label) loss[at_loss] = logloss_ref(rows.label[r], acc);
  }
}

}  // namespace ftrl_dev
