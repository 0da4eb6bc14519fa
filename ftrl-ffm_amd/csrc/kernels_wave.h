// kernels_wave.h -- scoring with one WAVE per row (or context, or candidate): the pieces every such kernel is
// built from, each written once, and the row kernel itself (src/eval/evaluate.cpp:23-33 over FFM::predict,
// src/model/ffm.cpp:24-70 with the stored w: no refresh, no update).
//
// A predict row has nothing to hide its serial sections behind when a whole workgroup waits on them
// (ffm_row_kernel<false, ..>: entries staged by one wave, the linear logit by one lane, the 741 terms of a
// 39-field row added in the reference's order by one wave, three barriers): six to eight rows per CU in flight,
// each ~20 us long.  Here a row is ONE wave and needs no barrier, so all 8192 rows of a block are resident at
// once (eight waves per SIMD) and a row's latency hides behind 31 others on its CU.
//
// Lanes: LPP consecutive lanes share a pair, each loads VPL vectors of four factors of both slots -- with
// LPP = k / 4 one load instruction fetches whole slots (a lane per pair reads 16 of the 64 bytes of a line per
// instruction).  The k-long dot runs lane after lane in factor order (DPP row_shr:1 hands the running value
// on), so it is the reference's sequential sum; the term is (dot*x1)*x2; the terms go through the wave's LDS
// into the strictly ordered sum (wave_sequential_prefix: one DPP add per term).  U steps of loads are in flight
// together.  Sharded / compact engines, LR, and k outside {4, 8, 16, 32, 64} keep ffm_row_kernel.
//
// The pieces, in the order a kernel uses them:
//   wave_lds             a wave's share of the dynamic LDS: its staged entries, and a batch of terms behind them
//   wave_stage_entries   remove_out_range, the survivors compacted into LDS in row order, the linear logit
//   WavePairCursor       a lane's walk over the pairs (a outer, b inner), 64 / LPP pairs per step
//   WaveTable<FMT>       where a slot's factors are: a training engine's [n][z][w] records, or a packed table of w
//   wave_pair_term       four products per vector, the factor-order dot across a pair's lanes, (dot*x1)*x2
//   wave_ordered_sum     a batch of terms into the running logit, strictly in order
// What differs between the kernels stays written in each: which steps gather at all and where a term goes (the
// U-step loop), what a row too long for a wave gets, and what is written at the end.  ffm_row_wave_kernel below,
// serve_context_kernel / serve_candidate_kernel (kernels_serve.h) and ffm_ablate_wave_kernel (kernels_ablate.h)
// are the users; the bit-exact pair order and summation order live here and nowhere else.
#pragma once
#include <hip/hip_fp16.h>

#include <type_traits>

#include "engine_types.h"
#include "kernels_touch.h"

namespace ftrl_dev {

constexpr int kPredRows = 4;     // rows (= waves) per workgroup
constexpr int kPredTerms = 256;  // terms staged per wave between two ordered sums (a multiple of 64)
constexpr int kPredLdsCap = 128; // entries of a row a wave stages at most (12 KB per workgroup: eight waves per SIMD)

__host__ __device__ inline size_t pred_lds_bytes(int lds_cap) {
  return static_cast<size_t>(kPredRows) * (static_cast<size_t>(lds_cap) * 16 + kPredTerms * 4);
}

// Six waves per SIMD, not the seven its registers would allow: with the rows streaming from host
// memory the upload kernel of the next block needs room beside this one (its 24 workgroups otherwise
// wait for a whole round of rows to retire): 51.9 -> 54.3 M rows/s with the H2D, resident unchanged.
#ifndef FFM_PRED_WAVES
#define FFM_PRED_WAVES 6
#endif
#define FFM_PRED_OCC __attribute__((amdgpu_waves_per_eu(FFM_PRED_WAVES, FFM_PRED_WAVES)))

// Pairs per step of a lane shape; U: steps of loads in flight together.
template <int LPP, int U>
constexpr int wave_pairs_per_step() {
  static_assert(LPP >= 1 && LPP <= 16 && (LPP & (LPP - 1)) == 0, "a pair's lanes sit inside one DPP row");
  static_assert(kPredTerms % 64 == 0, "whole prefix chunks");
  static_assert(kPredTerms % (64 / LPP * U) == 0, "a batch of terms is whole unrolled steps");
  return 64 / LPP;
}

// ---- the formats of a slot -------------------------------------------------------------------------------
enum { SERVE_NONE = 0, SERVE_F32 = 1, SERVE_F16 = 2 };  // ModelDev::lat_fmt

__device__ __forceinline__ float serve_dec16(unsigned short h) { return __half2float(__ushort_as_half(h)); }
// four consecutive halves as a lane loads them (8 bytes): element j in bits [16 j, 16 j + 16)
__device__ __forceinline__ float4 serve_dec16x4(uint2 r) {
  return make_float4(serve_dec16(static_cast<unsigned short>(r.x & 0xffffu)), serve_dec16(static_cast<unsigned short>(r.x >> 16)),
                     serve_dec16(static_cast<unsigned short>(r.y & 0xffffu)), serve_dec16(static_cast<unsigned short>(r.y >> 16)));
}
__device__ __forceinline__ float4 serve_widen(float4 r) { return r; }
__device__ __forceinline__ float4 serve_widen(uint2 r) { return serve_dec16x4(r); }

// FMT: SERVE_NONE (a training engine's [n][z][w] records: the w row of a feature's record), SERVE_F32 or
// SERVE_F16 (a packed table of w alone).  A vector is four factors as stored -- 16 bytes, or 8 of an fp16 table.
template <int FMT>
struct WaveTable {
  static_assert(FMT == SERVE_NONE || FMT == SERVE_F32 || FMT == SERVE_F16, "records, or a packed table of w");
  using Raw = typename std::conditional<FMT == SERVE_F16, uint2, float4>::type;
  const Raw *w;  // vector 0 of feature 0's w row
  int64_t rec4;  // vectors per feature
  int k4;        // vectors per slot
  __device__ __forceinline__ explicit WaveTable(const ModelDev &m) {
    const int64_t RL4 = m.row_len >> 2;
    w = reinterpret_cast<const Raw *>(m.lat) + (FMT == SERVE_NONE ? LAT_W * RL4 : 0);
    rec4 = FMT == SERVE_NONE ? 3 * RL4 : RL4;
    k4 = m.n_factors >> 2;
  }
  // vector 0 of the slot (feature `feat`, towards field `field`)
  __device__ __forceinline__ const Raw *slot(int feat, int field) const { return w + static_cast<int64_t>(feat) * rec4 + field * k4; }
};

// ---- a wave's LDS ----------------------------------------------------------------------------------------
struct WaveLds {
  int4 *E;       // [lds_cap] the staged survivors {feature, field, value bits, the kernel's own}
  float *terms;  // [n_terms] a batch of terms in pair order
};
// n_terms: kPredTerms (pred_lds_bytes), or 0 for a kernel that stages entries only (cand_ctx_lds_bytes)
__device__ __forceinline__ WaveLds wave_lds(char *smem, int wv, int lds_cap, int n_terms) {
  int4 *E = reinterpret_cast<int4 *>(smem + static_cast<size_t>(wv) * (static_cast<size_t>(lds_cap) * 16 + n_terms * 4));
  return {E, reinterpret_cast<float *>(E + lds_cap)};
}

// ---- entries: remove_out_range (ftrl_model.cpp:36-42, ffm.cpp:30-36), the survivors handed in row order to
// store(position, {feature, field, value bits, 0}, lin_w * value) with positions from nv on; the linear logit
// result + sum lin_w * x in row order (compute_linear_logit, ftrl_model.cpp:44-50) as a strictly sequential
// prefix.  What store wrote to LDS is the wave's to read when this returns.
template <typename Store>
__device__ __forceinline__ void wave_stage_entries(const ModelDev &m, const int *feat, const int *field, const float *val, int b,
                                                   int nnz, int lane, float &result, int &nv, Store store) {
  for (int base = 0; base < nnz; base += 64) {
    const int p = base + lane;
    int i = 0, f = 0;
    float x = 0.0f, lw = 0.0f;
    bool valid = false;
    if (p < nnz) {
      i = feat[b + p];
      f = field[b + p];
      x = val[b + p];
      valid = i >= 0 && i < m.n_feats && f >= 0 && f < m.n_fields;
    }
    if (valid) lw = m.lin_w[i];
    const unsigned long long mask = __ballot(valid);
    if (valid) store(nv + __popcll(mask & ((1ull << lane) - 1ull)), make_int4(i, f, __float_as_int(x), 0), lw * x);
    nv += __popcll(mask);
    // x + -0.0f == x bit for bit: idle lanes and erased entries add nothing
    const float run = wave_sequential_prefix(result, valid ? lw * x : -0.0f);
    result = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(run), 63));
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
}

// ---- pairs in the reference's order (a outer, b inner: ffm.cpp:52-66).  Group g of a step's 64 / LPP groups
// of lanes has pair number step * (64 / LPP) + g: entries pa < pb of nv.
struct WavePairCursor {
  int pa, pb;
  __device__ __forceinline__ void wrap(int nv) {
    while (pb >= nv) { pb = pb - nv + pa + 2; pa++; }
  }
  __device__ __forceinline__ void start(int g, int n_pairs, int nv) {
    pa = 0;
    pb = 1 + g;
    if (g < n_pairs) wrap(nv);
  }
  // the pair `pps` further on (the caller knows there is one)
  __device__ __forceinline__ void advance(int pps, int nv) {
    pb += pps;
    wrap(nv);
  }
};

// the value of the lane below (row_shr:1 inside the 16-lane DPP row; the first lane of a pair's
// group never uses it)
__device__ __forceinline__ float pred_lane_below(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xf, 0xf, false));
}

// ---- a pair's term.  Lane c of the pair's LPP lanes holds factors [4 VPL c, 4 VPL (c + 1)) of both slots as
// loaded; lane LPP - 1 returns (dot * xa) * xb with dot = ((0 + w0*v0) + w1*v1) + ... in factor order.
template <int LPP, int VPL, typename Raw>
__device__ __forceinline__ float wave_pair_term(const Raw (&x)[VPL], const Raw (&y)[VPL], int c, float xa, float xb) {
  float pr[VPL][4];
#pragma unroll
  for (int v = 0; v < VPL; v++) {
    const float4 xf = serve_widen(x[v]), yf = serve_widen(y[v]);
    pr[v][0] = xf.x * yf.x;
    pr[v][1] = xf.y * yf.y;
    pr[v][2] = xf.z * yf.z;
    pr[v][3] = xf.w * yf.w;
  }
  // stage t finalises the lanes c == t
  float dot = 0.0f;
#pragma unroll
  for (int t = 0; t < LPP; t++) {
    float in = LPP > 1 ? pred_lane_below(dot) : 0.0f;
    in = c == 0 ? 0.0f : in;
#pragma unroll
    for (int v = 0; v < VPL; v++) {
      in = in + pr[v][0];
      in = in + pr[v][1];
      in = in + pr[v][2];
      in = in + pr[v][3];
    }
    dot = in;
  }
  return dot * xa * xb;
}

// ---- result + terms[0] + terms[1] + ... + terms[cnt - 1], every addition in that order.  The caller fences
// between the lanes' stores to terms and this, and again before the next batch overwrites them.
__device__ __forceinline__ float wave_ordered_sum(float result, const float *terms, int cnt, int lane) {
  for (int t0 = 0; t0 < cnt; t0 += 64) {
    const float t = t0 + lane < cnt ? terms[t0 + lane] : -0.0f;
    const float run = wave_sequential_prefix(result, t);
    result = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(run), 63));
  }
  return result;
}

// ---- a row per wave, for a training engine's evaluation (FMT = SERVE_NONE) and a serving engine alike.
// A wave's LDS holds kPredLdsCap entries at most.  A training engine's rows may be longer (a device-resident
// block is not scanned on the host: its bound is the engine's max_row_nnz): those are left to ffm_row_kernel in
// a second launch, which returns at once for the others.  A serving engine has no such launch (create keeps
// max_row_nnz <= kPredLdsCap): everything a wave cannot stage is flagged like a row beyond max_row_nnz.
template <int FMT, int LPP, int VPL, int U>
__global__ __launch_bounds__(64 * kPredRows) FFM_PRED_OCC void ffm_row_wave_kernel(ModelDev m, Rows rows, Scratch s,
                                                                     int max_row_nnz, int lds_cap, float *out,
                                                                     int output_prob) {
  constexpr int PPS = wave_pairs_per_step<LPP, U>();
  using Raw = typename WaveTable<FMT>::Raw;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = wave_uniform(blockIdx.x * kPredRows + wv);
  if (r >= rows.n_rows) return;
  const WaveLds lds = wave_lds(smem, wv, lds_cap, kPredTerms);
  int4 *const E = lds.E;
  const int b = wave_uniform(rows.row_ptr[r]);
  const int nnz = wave_uniform(rows.row_ptr[r + 1]) - b;
  bool refused = nnz > max_row_nnz;  // beyond the validated capacity: flagged, NaN outputs
  if constexpr (FMT != SERVE_NONE) refused = refused || nnz > lds_cap;
  if (refused) {
    if (lane == 0) {
      atomicOr(s.err, ERR_ROW_TOO_LONG);
      const float nan = __int_as_float(0x7fc00000);
      s.loss[r] = static_cast<double>(nan);
      if (out) out[r] = nan;
    }
    return;
  }
  if constexpr (FMT == SERVE_NONE)
    if (nnz > lds_cap) return;  // (ffm_row_kernel's, in the launch behind this one)
  const WaveTable<FMT> table(m);

  float result = m.bias3[0];
  int nv = 0;
  wave_stage_entries(m, rows.feat, rows.field, rows.val, b, nnz, lane, result, nv, [&](int at, int4 en, float) { E[at] = en; });

  const int n_pairs = nv * (nv - 1) / 2;
  const int g = lane / LPP, c = lane - g * LPP;
  WavePairCursor cur;  // this lane's pair of the coming step: number q = step * PPS + g
  cur.start(g, n_pairs, nv);
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
        if (c == LPP - 1 && ok[u]) lds.terms[(st + u) * PPS + g] = term;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    result = wave_ordered_sum(result, lds.terms, cnt, lane);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  }

  if (lane == 0) {
    out[r] = output_prob ? sigmoid_ref(result) : result;
    if (rows.label) s.loss[r] = logloss_ref(rows.label[r], result);
  }
}

}  // namespace ftrl_dev
