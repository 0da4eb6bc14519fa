// kernels_ablate.h -- field ablation in one pass (include/ffm_engine.h "Field ablation"): for every row the
// n_fields + 1 logits "the row without field v" (v < n_fields) and "the row itself" (v = n_fields).
//   ffm_ablate_wave_kernel   ffm_row_wave_kernel's pieces (kernels_wave.h) with one more reader of what they
//                            stage -- the gathers and the k-long dots are made once per row.
//   ablate_loss_sum_kernel   loss_sum_kernel's arithmetic over each variant's slice of the loss scratch
//   ablate_hist_kernel       metric_hist_kernel's body (a second copy), one grid row (blockIdx.y) per variant
// The logit of the row without field v is the row's ordered sum with the terms that touch v left out; leaving a
// term out and adding -0.0f in its place are the same bits (x + -0.0f == x), so variant v is what the predict
// kernel returns for the block with those entries removed.  Lane v of the row's wave keeps variant v's running
// value: after the entries are staged it walks the survivors' stored lin_w * x products, after each batch of
// terms it walks the batch in pair order; every lane reads the same LDS address (a broadcast), compares the
// entry's field with its own number, and makes one dependent add per term.
#pragma once
#include "engine_types.h"
#include "kernels_metric.h"
#include "kernels_row.h"
#include "kernels_wave.h"

namespace ftrl_dev {

// One add of a variant's running value: the term, or -0.0f in the lanes whose field it touches.
__device__ __forceinline__ float ablate_add(float acc, bool drop, int term_bits) {
  return acc + __int_as_float(drop ? static_cast<int>(0x80000000u) : term_bits);
}
// What a walk has just read from LDS, made opaque to the compiler: left to itself it loads a term only in the
// lanes that will add it, behind a branch on the field -- two dependent LDS waits and two exec-mask branches per
// term instead of reads in flight together and a select.  (A loop that holds inline assembly is not unrolled on
// request either: the walks are unrolled by hand, four terms' reads ahead of their four dependent adds.)
__device__ __forceinline__ void ablate_pin(int &f, int &t) { asm volatile("" : "+v"(f), "+v"(t)); }
__device__ __forceinline__ void ablate_pin4(int (&f)[4], int (&t)[4]) {
  asm volatile("" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]));
}

// FMT: WaveTable's.  out[(n_fields + 1) * n_rows] variant-major; loss[(n_fields + 1) * loss_stride], written when labels came.
template <int FMT, int LPP, int VPL, int U>
__global__ __launch_bounds__(64 * kPredRows) FFM_PRED_OCC void ffm_ablate_wave_kernel(ModelDev m, Rows rows, int *err,
                                                                        int max_row_nnz, int lds_cap, float *out,
                                                                        double *loss, int loss_stride, int output_prob) {
  constexpr int PPS = wave_pairs_per_step<LPP, U>();
  using Raw = typename WaveTable<FMT>::Raw;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = wave_uniform(blockIdx.x * kPredRows + wv);
  if (r >= rows.n_rows) return;
  const WaveLds lds = wave_lds(smem, wv, lds_cap, kPredTerms);
  int4 *const E = lds.E;
  float *const terms = lds.terms;
  const int b = wave_uniform(rows.row_ptr[r]);
  const int nnz = wave_uniform(rows.row_ptr[r + 1]) - b;
  const int F = m.n_fields;  // (<= 64: one lane per variant v < F, lane 0 also variant F)
  const size_t at = static_cast<size_t>(lane) * rows.n_rows + r;  // variant `lane` of this row in out
  const size_t at_loss = static_cast<size_t>(lane) * loss_stride + r;
  const size_t whole = static_cast<size_t>(F) * rows.n_rows + r, whole_loss = static_cast<size_t>(F) * loss_stride + r;
  // beyond the validated capacity or what a wave stages (there is no second launch behind this one): flagged,
  // NaN in every variant
  if (nnz > max_row_nnz || nnz > lds_cap) {
    const float nan = __int_as_float(0x7fc00000);
    if (lane == 0) {
      atomicOr(err, ERR_ROW_TOO_LONG);
      out[whole] = nan;
      if (rows.label) loss[whole_loss] = static_cast<double>(nan);
    }
    if (lane < F) {
      out[at] = nan;
      if (rows.label) loss[at_loss] = static_cast<double>(nan);
    }
    return;
  }
  const WaveTable<FMT> table(m);

  // ---- entries: the survivors as {feature, field, value, lin_w * value}, the product for the variants' walk
  float result = m.bias3[0];
  int nv = 0;
  wave_stage_entries(m, rows.feat, rows.field, rows.val, b, nnz, lane, result, nv, [&](int at, int4 en, float lin) {
    en.w = __float_as_int(lin);
    E[at] = en;
  });

  // ---- the variants' linear part: lane v adds the survivors' products in order, field v's left out
  float acc = m.bias3[0];
  {
    int j = 0;
    for (; j + 4 <= nv; j += 4) {
      int f[4], t[4];
#pragma unroll
      for (int u = 0; u < 4; u++) { f[u] = E[j + u].y; t[u] = E[j + u].w; }
      ablate_pin4(f, t);
#pragma unroll
      for (int u = 0; u < 4; u++) acc = ablate_add(acc, f[u] == lane, t[u]);
    }
    for (; j < nv; j++) {
      int f = E[j].y, t = E[j].w;
      ablate_pin(f, t);
      acc = ablate_add(acc, f == lane, t);
    }
  }

  // ---- pairs, as the row kernel walks them
  const int n_pairs = nv * (nv - 1) / 2;
  const int g = lane / LPP, c = lane - g * LPP;
  WavePairCursor cur;
  cur.start(g, n_pairs, nv);
  int wa = 0, wb = 1;  // the variants' walker: the pair of the next term, the same in every lane
  for (int q0 = 0; q0 < n_pairs; q0 += kPredTerms) {
    const int cnt = min(kPredTerms, n_pairs - q0);
    for (int st = 0; st * PPS < cnt; st += U) {
      Raw x[U][VPL], y[U][VPL];
      float xa[U], xb[U];
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
        if (q + PPS < n_pairs) cur.advance(PPS, nv);
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        const float term = wave_pair_term<LPP, VPL>(x[u], y[u], c, xa[u], xb[u]);
        if (c == LPP - 1 && ok[u]) terms[(st + u) * PPS + g] = term;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    result = wave_ordered_sum(result, terms, cnt, lane);
    // ---- the variants' share of the batch: its terms in order, one `a` at a time (every term of an `a` shares
    // field(wa): hoisted), lane v leaving out what touches field v
    for (int t = 0; t < cnt;) {
      const bool drop_a = E[wa].y == lane;
      const int run = min(nv - wb, cnt - t);
      const float *const tt = terms + t;
      const int4 *const eb = E + wb;
      int j = 0;
      for (; j + 4 <= run; j += 4) {
        int f[4], tb[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { f[u] = eb[j + u].y; tb[u] = __float_as_int(tt[j + u]); }
        ablate_pin4(f, tb);
#pragma unroll
        for (int u = 0; u < 4; u++) acc = ablate_add(acc, drop_a | (f[u] == lane), tb[u]);
      }
      for (; j < run; j++) {
        int f = eb[j].y, tb = __float_as_int(tt[j]);
        ablate_pin(f, tb);
        acc = ablate_add(acc, drop_a | (f == lane), tb);
      }
      t += run;
      wb += run;
      if (wb >= nv) { wa++; wb = wa + 1; }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  }

  if (lane == 0) {
    out[whole] = output_prob ? sigmoid_ref(result) : result;
    if (rows.label) loss[whole_loss] = logloss_ref(rows.label[r], result);
  }
  if (lane < F) {
    out[at] = output_prob ? sigmoid_ref(acc) : acc;
    if (rows.label) loss[at_loss] = logloss_ref(rows.label[r], acc);
  }
}

// Variant blockIdx.y's loss sum: loss_sum_kernel's ranges, partial sums and order of additions over the
// variant's slice.  scratch: [variants][kLossParts + 1], a ticket counter behind each variant's partial sums.
__global__ __launch_bounds__(256) void ablate_loss_sum_kernel(int n_rows, const double *loss, int loss_stride, double *out,
                                                              double *scratch) {
  const unsigned v = blockIdx.y;
  loss_sum_body(n_rows, loss + static_cast<size_t>(v) * loss_stride, out + v, scratch + static_cast<size_t>(v) * (kLossParts + 1),
                blockIdx.x, gridDim.x);
}

// Variant blockIdx.y's scores into its own histogram: hist[variants][2 * kMetricBins + 1] = pos, neg, n_nan.
// metric_hist_kernel's body (kernels_metric.h: same bins, integer atomics, one atomic per distinct (bin, class)
// of a wave), written a second time: called from both kernels as one __device__ function it compiled
// metric_hist_kernel to the same registers but another instruction order, and that kernel stays what it is.
__global__ __launch_bounds__(kMetricThreads) void ablate_hist_kernel(int n_rows, const float *score, int is_prob,
                                                                     const int *label, unsigned long long *hist) {
  const size_t v = blockIdx.y;
  unsigned long long *const pos = hist + v * (2 * static_cast<size_t>(kMetricBins) + 1), *const neg = pos + kMetricBins;
  unsigned long long *const n_nan = pos + 2 * static_cast<size_t>(kMetricBins);
  const int r = blockIdx.x * kMetricThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  float p = 0.0f;
  int cls = 0;
  const bool live = r < n_rows;
  if (live) {
    const float s = score[v * n_rows + r];
    p = is_prob ? s : sigmoid_ref(s);
    cls = label[r] > 0 ? 1 : 0;
  }
  const bool is_nan = live && p != p;
  const unsigned long long nan_mask = __ballot(is_nan);
  if (nan_mask != 0ull && lane == __ffsll(nan_mask) - 1)
    __hip_atomic_fetch_add(n_nan, static_cast<unsigned long long>(__popcll(nan_mask)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const bool counts = live && !is_nan;
  const int key = counts ? metric_bin(p) * 2 + cls : -1;
  unsigned long long waiting = __ballot(counts);  // (wave-uniform: every lane walks the same turns)
  while (waiting != 0ull) {
    const int first = __ffsll(waiting) - 1;
    const int k0 = __builtin_amdgcn_readlane(key, first);  // the first waiting lane's key
    const unsigned long long same = __ballot(key == k0);
    if (lane == first)
      __hip_atomic_fetch_add(((k0 & 1) ? pos : neg) + (k0 >> 1), static_cast<unsigned long long>(__popcll(same)),
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    waiting &= ~same;
  }
}

}  // namespace ftrl_dev
