// kernels_serve.h -- a SERVING engine's device code (include/ffm_engine.h "Serving engines"): the model is
// the bias, lin_w and a latent table of w ALONE, [n_feats][n_fields * n_factors] elements of 4 bytes (the
// training engine's fp32 bits) or 2 (IEEE binary16) -- no n, no z, no record stride.
// Rows are scored by ffm_row_wave_kernel<SERVE_F32 | SERVE_F16> (kernels_wave.h: WaveTable<FMT> is the address
// of a slot in that table and the conversion of what was loaded).  Here:
//   serve_context_kernel / serve_candidate_kernel   one context against many candidates, from the same pieces
//   serve_init_kernel      the create-time contents: the training engine's draw, rounded to the format
//   serve_dense_copy_kernel / serve_rows_copy_kernel   packed table <-> the fp32 staging buffer
//   serve_pack_kernel       a training engine's stored bias, lin_w and w into a serving engine, counted
// The fp16 rule is the hardware's conversion pair (v_cvt_f16_f32 / v_cvt_f32_f16 with 16-bit denormals on and
// no overflow clamp): round to nearest even, subnormals kept, beyond the half range +-inf, NaN stays NaN;
// decoding is exact.  tests/test_gpu_serve.py pins it against numpy's astype(float16).
#pragma once
#include <hip/hip_fp16.h>

#include "engine_types.h"
#include "init_rng.h"
#include "kernels_wave.h"

namespace ftrl_dev {

// (SERVE_NONE / SERVE_F32 / SERVE_F16 and the decoding half of the pair, serve_dec16 / serve_dec16x4: kernels_wave.h)
__device__ __forceinline__ unsigned short serve_enc16(float x) { return __half_as_ushort(__float2half_rn(x)); }
__device__ __forceinline__ uint2 serve_enc16x4(float4 w) {
  return make_uint2(static_cast<unsigned>(serve_enc16(w.x)) | (static_cast<unsigned>(serve_enc16(w.y)) << 16),
                    static_cast<unsigned>(serve_enc16(w.z)) | (static_cast<unsigned>(serve_enc16(w.w)) << 16));
}

// Element `idx` of the packed table, whatever its format.
__device__ __forceinline__ float serve_load_elem(const ModelDev &m, int64_t idx) {
  return m.lat_fmt == SERVE_F16 ? serve_dec16(reinterpret_cast<const unsigned short *>(m.lat)[idx]) : m.lat[idx];
}
__device__ __forceinline__ void serve_store_elem(const ModelDev &m, int64_t idx, float w) {
  if (m.lat_fmt == SERVE_F16) reinterpret_cast<unsigned short *>(m.lat)[idx] = serve_enc16(w);
  else m.lat[idx] = w;
}

// ---- one context against many candidates (include/ffm_engine.h "Scoring candidates") ---------------
//
// A candidate's score is ffm_row_wave_kernel's on the row [context entries ..., candidate entries ...].  What
// every candidate of a request shares is made once per request by serve_context_kernel and read by each
// candidate's wave in serve_candidate_kernel: the context's survivors as staged entries, the running value
// after the bias and the context's linear terms, and the TERM of every context x context pair (the sum itself
// cannot be shared: in pair order those terms interleave with the context x candidate ones).  The candidate's
// wave feeds a stored term into the same ordered sum at the pair's position in the concatenated row and issues
// no gathers for it.
struct CandCtx {
  int4 *ent;      // [n_req][ctx_cap] the context's survivors {id, field, val bits, 0}, in order
  int2 *head;     // [n_req] {survivors, or kCandVoid; bits of the linear prefix}
  float *terms;   // [n_req][ctx_cap (ctx_cap - 1) / 2] pair (a, b) of nc survivors at a nc - a (a + 1) / 2 + (b - a - 1)
  int *cand_req;  // [n_cand] the request of every candidate
  int ctx_cap;    // entries of a context at most (raw, before erasure)
};
constexpr int kCandVoid = -1;  // head.x of a request whose context is too long: its candidates are NaN

__host__ __device__ inline size_t cand_ctx_lds_bytes(int lds_cap) {
  return static_cast<size_t>(kPredRows) * static_cast<size_t>(lds_cap) * 16;
}
__host__ __device__ inline int64_t cand_terms_stride(int ctx_cap) {
  return static_cast<int64_t>(ctx_cap) * (ctx_cap - 1) / 2;
}

// One wave per request, kPredRows requests per workgroup.  Also writes the request of each of its candidates
// (cand_req_ptr[r] .. cand_req_ptr[r + 1], kept inside [0, n_cand)).
template <int FMT, int LPP, int VPL, int U>
__global__ __launch_bounds__(64 * kPredRows) FFM_PRED_OCC void serve_context_kernel(ModelDev m, int n_req, const int *ctx_ptr,
                                                                      const int *field, const int *feat, const float *val,
                                                                      const int *cand_req_ptr, int n_cand, CandCtx cx,
                                                                      int max_row_nnz, int lds_cap, int *err) {
  static_assert(FMT == SERVE_F32 || FMT == SERVE_F16, "a packed table of w alone");
  constexpr int PPS = wave_pairs_per_step<LPP, U>();
  using Raw = typename WaveTable<FMT>::Raw;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = wave_uniform(blockIdx.x * kPredRows + wv);
  if (r >= n_req) return;
  int4 *const E = wave_lds(smem, wv, lds_cap, 0).E;  // (entries only: the terms go to cx.terms)
  const int c0 = wave_uniform(cand_req_ptr[r]), c1 = wave_uniform(cand_req_ptr[r + 1]);
  for (int cc = max(c0, 0) + lane; cc < min(c1, n_cand); cc += 64) cx.cand_req[cc] = r;
  const int b = wave_uniform(ctx_ptr[r]);
  const int nnz = wave_uniform(ctx_ptr[r + 1]) - b;
  if (nnz > cx.ctx_cap || nnz > max_row_nnz || nnz > lds_cap) {
    if (lane == 0) {
      atomicOr(err, ERR_ROW_TOO_LONG);
      cx.head[r] = make_int2(kCandVoid, 0);
    }
    return;
  }
  const WaveTable<FMT> table(m);
  int4 *const ent = cx.ent + static_cast<int64_t>(r) * cx.ctx_cap;

  // ---- entries: as the row kernel stages a row's, and a copy for the candidates' waves
  float result = m.bias3[0];
  int nv = 0;
  wave_stage_entries(m, feat, field, val, b, nnz, lane, result, nv, [&](int at, int4 en, float) { E[at] = en; ent[at] = en; });
  if (lane == 0) cx.head[r] = make_int2(nv, __float_as_int(result));

  // ---- the context x context terms in pair order, each as the row kernel computes it
  const int n_pairs = nv * (nv - 1) / 2;
  float *const T = cx.terms + static_cast<int64_t>(r) * cand_terms_stride(cx.ctx_cap);
  const int g = lane / LPP, c = lane - g * LPP;
  WavePairCursor cur;
  cur.start(g, n_pairs, nv);
  for (int st = 0; st * PPS < n_pairs; st += U) {
    Raw x[U][VPL], y[U][VPL];
    float xa[U], xb[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int q = (st + u) * PPS + g;
      ok[u] = q < n_pairs;
      const int a = ok[u] ? cur.pa : 0, bb = ok[u] ? cur.pb : 1;  // (n_pairs > 0 here: entries 0 and 1 exist)
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
      if (c == LPP - 1 && ok[u]) T[(st + u) * PPS + g] = term;
    }
  }
}

// One wave per candidate, kPredRows candidates per workgroup: the row kernel on the concatenated row, with the
// request's staged survivors copied in place of the context's entries, the linear prefix continued, and the
// stored term loaded (4 bytes, one lane, no gathers) for every pair whose members are both context.
template <int FMT, int LPP, int VPL, int U>
__global__ __launch_bounds__(64 * kPredRows) FFM_PRED_OCC void serve_candidate_kernel(ModelDev m, int n_req, const int *ctx_ptr,
                                                                        CandCtx cx, Rows rows, int max_row_nnz, int lds_cap,
                                                                        int *err, float *out, int output_prob) {
  static_assert(FMT == SERVE_F32 || FMT == SERVE_F16, "a packed table of w alone");
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
  const int req = wave_uniform(cx.cand_req[r]);
  const bool known = req >= 0 && req < n_req;  // (a candidate no request lists: NaN)
  const int2 head = known ? cx.head[req] : make_int2(kCandVoid, 0);
  const int nc = wave_uniform(head.x);
  const int raw = known ? wave_uniform(ctx_ptr[req + 1]) - wave_uniform(ctx_ptr[req]) + nnz : 0;
  // the row's raw length against the validated capacity and what a wave stages, as in the row kernel
  if (nc == kCandVoid || raw > max_row_nnz || raw > lds_cap) {
    if (lane == 0) {
      atomicOr(err, ERR_ROW_TOO_LONG);
      out[r] = __int_as_float(0x7fc00000);
    }
    return;
  }
  const WaveTable<FMT> table(m);

  // ---- entries: the request's survivors as staged, then the candidate's behind them; the linear logit goes
  // on from the context's prefix
  const int4 *const ent = cx.ent + static_cast<int64_t>(req) * cx.ctx_cap;
  for (int p = lane; p < nc; p += 64) E[p] = ent[p];
  float result = __int_as_float(wave_uniform(head.y));
  int nv = nc;
  wave_stage_entries(m, rows.feat, rows.field, rows.val, b, nnz, lane, result, nv, [&](int at, int4 en, float) { E[at] = en; });

  // ---- pairs over the concatenated survivors
  const int n_pairs = nv * (nv - 1) / 2;
  const float *const T = cx.terms + static_cast<int64_t>(req) * cand_terms_stride(cx.ctx_cap);
  const int g = lane / LPP, c = lane - g * LPP;
  WavePairCursor cur;
  cur.start(g, n_pairs, nv);
  for (int q0 = 0; q0 < n_pairs; q0 += kPredTerms) {
    const int cnt = min(kPredTerms, n_pairs - q0);
    for (int st = 0; st * PPS < cnt; st += U) {
      Raw x[U][VPL], y[U][VPL];
      float xa[U], xb[U], kept[U];
      bool ok[U], shared[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int q = q0 + (st + u) * PPS + g;
        ok[u] = q < n_pairs;
        const int a = ok[u] ? cur.pa : 0, bb = ok[u] ? cur.pb : (nv > 1 ? 1 : 0);
        shared[u] = ok[u] && bb < nc;  // (a < bb: both members are the context's)
        const int4 ea = E[a], eb = E[bb];
        xa[u] = __int_as_float(ea.z);
        xb[u] = __int_as_float(eb.z);
        kept[u] = 0.0f;
#pragma unroll
        for (int v = 0; v < VPL; v++) { x[u][v] = Raw{}; y[u][v] = Raw{}; }
        if (shared[u]) {
          if (c == LPP - 1) kept[u] = T[a * nc - a * (a + 1) / 2 + (bb - a - 1)];
        } else if (ok[u]) {
          const Raw *va = table.slot(ea.x, eb.y) + c * VPL, *vb = table.slot(eb.x, ea.y) + c * VPL;
#pragma unroll
          for (int v = 0; v < VPL; v++) { x[u][v] = va[v]; y[u][v] = vb[v]; }
        }
        if (q + PPS < n_pairs) cur.advance(PPS, nv);
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        const float term = wave_pair_term<LPP, VPL>(x[u], y[u], c, xa[u], xb[u]);
        if (c == LPP - 1 && ok[u]) lds.terms[(st + u) * PPS + g] = shared[u] ? kept[u] : term;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    result = wave_ordered_sum(result, lds.terms, cnt, lane);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  }

  if (lane == 0) out[r] = output_prob ? sigmoid_ref(result) : result;
}

// ---- the small streaming kernels -----------------------------------------------------------------

// Create-time contents: the element a training engine would draw (same seed, same index), in the format.
__global__ void serve_init_kernel(ModelDev m, float mean, float stddev, uint64_t seed) {
  const int64_t n_lat = static_cast<int64_t>(m.n_feats) * m.row_len;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  const int64_t t0 = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  for (int64_t idx = t0; idx < n_lat; idx += stride)
    serve_store_elem(m, idx, ftrl_rng::init_weight(seed, 1, idx, mean, stddev));
  for (int64_t i = t0; i < m.n_feats; i += stride) m.lin_w[i] = ftrl_rng::init_weight(seed, 0, i, mean, stddev);
}

// Features [feat0, feat0 + nf) of the packed table <-> dense[nf][row_len] fp32 (lat_component_copy_kernel's
// analogue: the table IS the reference's save order, so it is one contiguous range).
__global__ void serve_dense_copy_kernel(ModelDev m, float *dense, int64_t feat0, int64_t nf, int to_dense) {
  const int64_t total = nf * m.row_len, first = feat0 * m.row_len;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; idx < total; idx += stride) {
    if (to_dense) dense[idx] = serve_load_elem(m, first + idx);
    else serve_store_elem(m, first + idx, dense[idx]);
  }
}

// The same for a list of features: ids[j] <-> dense[j][row_len] (lat_rows_copy_kernel's analogue).
__global__ void serve_rows_copy_kernel(ModelDev m, float *dense, const int *ids, int64_t nf, int to_dense) {
  const int64_t RL = m.row_len, total = nf * RL;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; idx < total; idx += stride) {
    const int64_t j = idx / RL;
    const int i = ids[j];
    const bool in = i >= 0 && i < m.n_feats;
    const int64_t at = static_cast<int64_t>(i) * RL + (idx - j * RL);
    if (to_dense) dense[idx] = in ? serve_load_elem(m, at) : 0.0f;
    else if (in) serve_store_elem(m, at, dense[idx]);
  }
}

// ffm_engine_pack_weights: src (a whole training engine's records) -> dst (packed), one pass.  Every
// counter on a 64-byte line of its own (kPackLine 64-bit words apart), one atomic per counter and wave.
enum { PK_LATENT = 0, PK_INEXACT = 1, PK_TO_INF = 2, PK_TO_ZERO = 3, PK_COUNT = 4 };
constexpr int kPackLine = 8;
constexpr int kPackThreads = 256;

__device__ __forceinline__ unsigned long long serve_wave_sum(unsigned v) {
  unsigned long long s = v;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  return s;
}

template <int FMT>
__global__ __launch_bounds__(kPackThreads) void serve_pack_kernel(ModelDev src, ModelDev dst, unsigned long long *counters) {
  const int64_t T = static_cast<int64_t>(gridDim.x) * kPackThreads;
  const int64_t g = static_cast<int64_t>(blockIdx.x) * kPackThreads + threadIdx.x;
  for (int64_t i = g; i < src.n_feats; i += T) dst.lin_w[i] = __builtin_nontemporal_load(src.lin_w + i);
  if (g == 0) dst.bias3[0] = src.bias3[0];
  // item = four consecutive elements of a feature's w row (row_len is a multiple of 4: n_factors is)
  const int64_t RL4 = src.row_len / 4, total = static_cast<int64_t>(src.n_feats) * RL4;
  const float4 *const rec = reinterpret_cast<const float4 *>(src.lat);
  unsigned part[PK_COUNT] = {0u, 0u, 0u, 0u};
  for (int64_t it = g; it < total; it += T) {
    const int64_t f = it / RL4, v = it - f * RL4;
    const float4 w = load_nt(rec + f * 3 * RL4 + LAT_W * RL4 + v);
    if (FMT == SERVE_F32) {
      store_nt(reinterpret_cast<float4 *>(dst.lat) + it, w);
    } else {
      const uint2 h = serve_enc16x4(w);
      reinterpret_cast<uint2 *>(dst.lat)[it] = h;
      const float4 d = serve_dec16x4(h);
      const float ws[4] = {w.x, w.y, w.z, w.w}, ds[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const bool nan = ws[c] != ws[c];
        part[PK_INEXACT] += (!nan && __float_as_uint(ds[c]) != __float_as_uint(ws[c])) ? 1u : 0u;
        part[PK_TO_INF] += (!nan && !isinf(ws[c]) && isinf(ds[c])) ? 1u : 0u;
        part[PK_TO_ZERO] += (!nan && ws[c] != 0.0f && ds[c] == 0.0f) ? 1u : 0u;
      }
    }
    part[PK_LATENT] += 4u;
  }
#pragma unroll
  for (int k = 0; k < PK_COUNT; k++) {
    const unsigned long long sum = serve_wave_sum(part[k]);
    if ((threadIdx.x & 63) == 0 && sum != 0ull)
      __hip_atomic_fetch_add(counters + k * kPackLine, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace ftrl_dev
