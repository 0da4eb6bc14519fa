// kernels_ablate_pairs.h -- pair ablation in one pass (include/ffm_engine.h "Pair ablation"): for every row the
// V + 1 logits "the row without the interaction of fields f and g" (V = F (F + 1) / 2 unordered pairs f <= g, the
// diagonal included) and "the row itself" (variant V).
//   ffm_ablate_pairs_kernel   ffm_ablate_wave_kernel's structure (kernels_ablate.h): one wave per row, the pieces
//                             of kernels_wave.h as they are, the gathers and the k-long dots made once per row.
// The loss sums and the histograms are ablate_loss_sum_kernel and ablate_hist_kernel (kernels_ablate.h), unchanged,
// launched with gridDim.y = V + 1.
//
// Variant (f, g) of a row is the prediction kernel's ordered sum -- bias, the survivors' linear products, then the
// pair terms in the row kernel's pair order -- with every term whose two entries have the fields {f, g} left out
// (f == g: the terms between two entries of field f).  Linear terms never leave.  Leaving a term out and adding
// -0.0f in its place are the same bits (x + -0.0f == x).  A term's two fields name exactly one variant,
//   pair_index(f, g) = f F - f (f - 1) / 2 + (g - f)      for f <= g,
// so every term is left out of exactly one variant.
//
// Where the variants live: lane l keeps the running values of variants l, l + 64, l + 128, ... in R registers
// (R >= ceil(V / 64) is a template bound -- 13 at 39 fields, 33 at 64 -- so that every index is a constant and
// nothing goes to scratch; engine_select.h picks the bound).  Per term the dropped variant pv is the same in
// every lane: accumulator r of lane l adds the term unless pv == l + 64 r, and then it adds -0.0f -- a compare, a
// select and an add per accumulator, no branch, and the R chains of a lane are independent of each other.  The
// linear part needs no walk of its own: nothing of it is ever left out, so every variant's value after the
// entries is the row's own strictly ordered prefix, which wave_stage_entries returns.
//
// How the definition is checked with the yardsticks that exist (no new oracle code).  Take a block in which every
// feature id occurs under one field only, and a model whose bias is not -0.0.  Then variant (f, g) equals
// predict_batch of the same block on a model whose vec_w[id, slot g, :] is +0.0 for every id of field f: the
// k-long dot of every term between an entry of f and an entry of g has a zeroed factor in each product, so the
// term is +-0.0 -- and a running sum that starts at a bias other than -0.0 can never be -0.0 (x + y is -0.0 only
// for x == y == -0.0), so adding +-0.0 to it changes no bit, exactly like leaving the term out.  No other term
// reads a zeroed slot: slot g of an id of field f is read only against an entry of field g.  The CPU checker's
// predict_batch and a twin engine's predict_batch on such weights are therefore the expected values of the tests
// (engine.py: drop_pair_weights).
#pragma once
#include "engine_types.h"
#include "kernels_ablate.h"
#include "kernels_row.h"
#include "kernels_wave.h"

namespace ftrl_dev {

constexpr int kPairFields = 64;  // n_fields at the most: V = 2080 variants, 33 rounds of 64 lanes

// pair_index(f, g) = pair_base(F, f) + g for f <= g
__host__ __device__ inline int pair_base(int F, int f) { return f * F - f * (f - 1) / 2 - f; }
__host__ __device__ inline int pair_variants(int F) { return F * (F + 1) / 2; }

// One term into a lane's R running values.  d = pv - lane: accumulator r holds variant lane + 64 r, the dropped one
// iff d == 64 r (d < 0 or no multiple of 64: none of this lane's).
template <int R>
__device__ __forceinline__ void pair_ablate_add(float (&acc)[R], int d, int term_bits) {
#pragma unroll
  for (int r = 0; r < R; r++) acc[r] = ablate_add(acc[r], d == 64 * r, term_bits);
}
// ablate_pin4 (kernels_ablate.h) for the three words a term's walk reads: the second entry's field and pair_base,
// the term -- four terms' reads in flight ahead of their 4 R adds.
__device__ __forceinline__ void pair_pin(int &f, int &b, int &t) { asm volatile("" : "+v"(f), "+v"(b), "+v"(t)); }
__device__ __forceinline__ void pair_pin4(int (&f)[4], int (&b)[4], int (&t)[4]) {
  asm volatile("" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]),
               "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]));
}

// FMT: WaveTable's; R: the accumulators of a lane, 64 R >= V.  out[(V + 1) * n_rows] variant-major;
// loss[(V + 1) * loss_stride], written when labels came.  No workgroup waits for another; every store is guarded
// by the row count (the early return) and by v < V.
template <int FMT, int LPP, int VPL, int U, int R>
__global__ __launch_bounds__(64 * kPredRows) void ffm_ablate_pairs_kernel(ModelDev m, Rows rows, int *err, int max_row_nnz,
                                                                          int lds_cap, float *out, double *loss,
                                                                          int loss_stride, int output_prob) {
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
  const int F = m.n_fields;  // (<= kPairFields, and 64 R >= V: the engine checks both before it launches)
  const int V = pair_variants(F);
  const size_t whole = static_cast<size_t>(V) * rows.n_rows + r, whole_loss = static_cast<size_t>(V) * loss_stride + r;
  // beyond the validated capacity or what a wave stages (there is no second launch behind this one): flagged,
  // NaN in every variant
  if (nnz > max_row_nnz || nnz > lds_cap) {
    const float nan = __int_as_float(0x7fc00000);
    if (lane == 0) {
      atomicOr(err, ERR_ROW_TOO_LONG);
      out[whole] = nan;
      if (rows.label) loss[whole_loss] = static_cast<double>(nan);
    }
    for (int v = lane; v < V; v += 64) {
      out[static_cast<size_t>(v) * rows.n_rows + r] = nan;
      if (rows.label) loss[static_cast<size_t>(v) * loss_stride + r] = static_cast<double>(nan);
    }
    return;
  }
  const WaveTable<FMT> table(m);

  // ---- entries: the survivors as {feature, field, value, pair_base(field)}
  float result = m.bias3[0];
  int nv = 0;
  wave_stage_entries(m, rows.feat, rows.field, rows.val, b, nnz, lane, result, nv, [&](int at, int4 en, float) {
    en.w = pair_base(F, en.y);
    E[at] = en;
  });

  // ---- the variants' linear part: nothing of it is ever left out
  float acc[R];
#pragma unroll
  for (int i = 0; i < R; i++) acc[i] = result;

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
    // ---- the variants' share of the batch: its terms in order, one `a` at a time (field(wa) and its pair_base
    // hoisted, as scalars).  The dropped variant of a term is the same in every lane: scalar arithmetic, then
    // one subtraction per term and a compare, a select and an add per accumulator.
    for (int t = 0; t < cnt;) {
      const int4 ea = E[wa];
      const int fa = wave_uniform(ea.y), base_a = wave_uniform(ea.w);
      const int run = min(nv - wb, cnt - t);
      const float *const tt = terms + t;
      const int4 *const eb = E + wb;
      int j = 0;
      for (; j + 4 <= run; j += 4) {
        int f[4], bs[4], tb[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const int4 e2 = eb[j + u];
          f[u] = e2.y;
          bs[u] = e2.w;
          tb[u] = __float_as_int(tt[j + u]);
        }
        pair_pin4(f, bs, tb);
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const int fb = wave_uniform(f[u]), base_b = wave_uniform(bs[u]);
          const int pv = fa <= fb ? base_a + fb : base_b + fa;
          pair_ablate_add<R>(acc, pv - lane, tb[u]);
        }
      }
      for (; j < run; j++) {
        const int4 e2 = eb[j];
        int f = e2.y, bs = e2.w, tb = __float_as_int(tt[j]);
        pair_pin(f, bs, tb);
        const int fb = wave_uniform(f), base_b = wave_uniform(bs);
        const int pv = fa <= fb ? base_a + fb : base_b + fa;
        pair_ablate_add<R>(acc, pv - lane, tb);
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
#pragma unroll
  for (int i = 0; i < R; i++) {
    const int v = lane + 64 * i;
    if (v < V) {
      out[static_cast<size_t>(v) * rows.n_rows + r] = output_prob ? sigmoid_ref(acc[i]) : acc[i];
      if (rows.label) loss[static_cast<size_t>(v) * loss_stride + r] = logloss_ref(rows.label[r], acc[i]);
    }
  }
}

}  // namespace ftrl_dev
