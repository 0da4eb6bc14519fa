// kernels_serve8.h -- the `f8` serving format (include/ffm_engine.h "Serving engines", FFM_FLAG_SERVE_F8):
// a latent table of OCP e4m3fn bytes with one power-of-two scale per feature row, and the kernels that read
// and write it.
//
// A feature's row is 16 + round_up(row_len, 16) bytes: bytes 0-3 the scale (fp32, 2^s), bytes 4-15 zero,
// element j at byte 16 + j, padding zero.  A slot of k factors is therefore k bytes, aligned to min(k, 16).
//
//   ffm_row8_wave_kernel   a row per wave (kernels_wave.h's pieces: the pair order and the ordered sum live
//                          there), but a lane shape of its own.  ffm_row_wave_kernel gives every lane one
//                          "vector" of four factors; on this table that is a 4-byte load, and the kernel is
//                          bound by the number of gathers in flight, not by their bytes.  Here a lane loads
//                          up to 16 factors in ONE load of 4, 8 or 16 bytes: k <= 16 is a pair per lane, 64
//                          pairs per step (16 with fp32 or fp16 at k = 16), k = 32 / 64 are 2 / 4 lanes per
//                          pair chained through pred_lane_below.  The scale words are gathered once per
//                          ENTRY while it is staged and ride in the staged int4's fourth word, so a pair
//                          costs two gathers and nothing else.  Decoding is v_cvt_pk_f32_fp8 and one
//                          multiply by the scale (exact: a power of two, and the format's lower clamp keeps
//                          every product normal or zero); the dot is wave_pair_term's on the decoded values.
//   serve8_encode_row      the encoder, written once: a group of 16 or 64 lanes owns a feature row, reduces
//                          max |w| over its finite elements, derives s, encodes four elements per
//                          v_cvt_pk_fp8_f32 pair, stores 16 bytes per lane, writes the head and the padding.
//                          A lane keeps its first 16 elements in registers; what a row has beyond
//                          16 * group elements is read a second time (out of L2).
//   serve_pack8_kernel / serve8_init_kernel / serve8_encode_kernel   its three callers: a training engine's
//                          stored w, the create-time draws, fp32 rows from the staging buffer
//   serve8_decode_kernel   table -> fp32 rows in the staging buffer, through the row kernel's decode
//
// Every kernel here is compiled without the packed fp32 instructions (FFM_SERVE8_FN).  The decode multiplies
// the two halves of every v_cvt_pk_f32_fp8 result by one scale, which the compiler otherwise turns into
// v_pk_mul_f32 with the scale broadcast (op_sel_hi): the one place in this project where that form would be
// emitted, on a path whose contract is bit-for-bit equality with plain v_mul_f32 code.  Keeping the new path on
// the scalar multiplies every other kernel here already uses costs nothing that shows: the resource report of
// both builds is in profiles/serve_f8.md.  -DFFM_SERVE8_FN= builds the other variant.
#pragma once
#include "engine_types.h"
#include "init_rng.h"
#include "kernels_serve.h"
#include "kernels_wave.h"

namespace ftrl_dev {

#ifndef FFM_SERVE8_FN
#define FFM_SERVE8_FN __attribute__((target("no-packed-fp32-ops")))
#endif

typedef float serve8_f2 __attribute__((ext_vector_type(2)));

constexpr int kServe8Head = 16;  // bytes in front of a row's elements: the scale word and twelve zero bytes
__host__ __device__ inline int64_t serve8_stride(int row_len) { return kServe8Head + ((static_cast<int64_t>(row_len) + 15) & ~15ll); }

// ---- decode: four bytes as a lane loads them (element j in bits [8 j, 8 j + 8)) times the row's scale ------
__device__ __forceinline__ float4 serve8_dec4(unsigned q, float scale) {
  const serve8_f2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(q), false);
  const serve8_f2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(q), true);
  return make_float4(lo.x * scale, lo.y * scale, hi.x * scale, hi.y * scale);
}

// What a lane loads of a slot: B = min(k, 16) bytes.
template <int B> struct Serve8Raw;
template <> struct Serve8Raw<4> { using type = unsigned; };
template <> struct Serve8Raw<8> { using type = uint2; };
template <> struct Serve8Raw<16> { using type = uint4; };
__device__ __forceinline__ void serve8_widen(unsigned r, float s, float4 (&o)[1]) { o[0] = serve8_dec4(r, s); }
__device__ __forceinline__ void serve8_widen(uint2 r, float s, float4 (&o)[2]) {
  o[0] = serve8_dec4(r.x, s);
  o[1] = serve8_dec4(r.y, s);
}
__device__ __forceinline__ void serve8_widen(uint4 r, float s, float4 (&o)[4]) {
  o[0] = serve8_dec4(r.x, s);
  o[1] = serve8_dec4(r.y, s);
  o[2] = serve8_dec4(r.z, s);
  o[3] = serve8_dec4(r.w, s);
}

// ---- a row per wave on the f8 table.  K: n_factors; U: steps of loads in flight together.
// Registers (what the compiler reports for gfx950 at -O3, no scratch anywhere): a step in flight is 2 * B / 4
// raw words plus two values and two scales -- 12 VGPRs at k >= 16 -- and a term's decode wants 32 more there.
//   k = 4, 8    U = 4: 45 and 52 VGPRs, eight waves per SIMD;
//   k = 16      U = 4: 77 VGPRs, six waves per SIMD -- the occupancy ffm_row_wave_kernel pins, with 256 pairs of
//               a row in flight per wave where that kernel has 64;
//   k = 32, 64  U = 2 (U = 4 is 88 VGPRs, five waves): 2 x 64 sixteen-byte loads per slot side in flight, which is
//               what ffm_row_wave_kernel keeps at k = 32 and twice its k = 64.
// No occupancy attribute: the compiler's counts already sit at or above FFM_PRED_WAVES, and pinning k = 4 / 8
// down to six waves would only take resident rows away.
template <int K, int U>
__global__ __launch_bounds__(64 * kPredRows) FFM_SERVE8_FN void ffm_row8_wave_kernel(ModelDev m, Rows rows, Scratch s, int max_row_nnz,
                                                                                     int lds_cap, float *out, int output_prob) {
  static_assert(K == 4 || K == 8 || K == 16 || K == 32 || K == 64, "a slot is one load of a lane, or 2 / 4 lanes' loads");
  constexpr int LPP = K > 16 ? K / 16 : 1, B = K > 16 ? 16 : K, VPL = B / 4;
  constexpr int PPS = wave_pairs_per_step<LPP, U>();
  using Raw = typename Serve8Raw<B>::type;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = wave_uniform(blockIdx.x * kPredRows + wv);
  if (r >= rows.n_rows) return;
  const WaveLds lds = wave_lds(smem, wv, lds_cap, kPredTerms);
  int4 *const E = lds.E;
  const int b = wave_uniform(rows.row_ptr[r]);
  const int nnz = wave_uniform(rows.row_ptr[r + 1]) - b;
  if (nnz > max_row_nnz || nnz > lds_cap) {  // as on the other serving formats: flagged, NaN outputs
    if (lane == 0) {
      atomicOr(s.err, ERR_ROW_TOO_LONG);
      const float nan = __int_as_float(0x7fc00000);
      s.loss[r] = static_cast<double>(nan);
      if (out) out[r] = nan;
    }
    return;
  }
  const char *const tab = reinterpret_cast<const char *>(m.lat);
  const int64_t stride = serve8_stride(m.row_len);

  // ---- entries, each with its feature's scale word beside it
  float result = m.bias3[0];
  int nv = 0;
  wave_stage_entries(m, rows.feat, rows.field, rows.val, b, nnz, lane, result, nv, [&](int at, int4 en, float) {
    en.w = *reinterpret_cast<const int *>(tab + en.x * stride);
    E[at] = en;
  });

  const int n_pairs = nv * (nv - 1) / 2;
  const int g = lane / LPP, c = lane - g * LPP;
  const int in_slot = kServe8Head + c * B;  // this lane's bytes of a slot, from the row's first byte
  WavePairCursor cur;
  cur.start(g, n_pairs, nv);
  for (int q0 = 0; q0 < n_pairs; q0 += kPredTerms) {
    const int cnt = min(kPredTerms, n_pairs - q0);
    for (int st = 0; st * PPS < cnt; st += U) {
      Raw x[U], y[U];
      float xa[U], xb[U], sa[U], sb[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int q = q0 + (st + u) * PPS + g;
        ok[u] = q < n_pairs;
        const int a = ok[u] ? cur.pa : 0, bb = ok[u] ? cur.pb : (nv > 1 ? 1 : 0);
        const int4 ea = E[a], eb = E[bb];
        xa[u] = __int_as_float(ea.z);
        xb[u] = __int_as_float(eb.z);
        sa[u] = __int_as_float(ea.w);
        sb[u] = __int_as_float(eb.w);
        x[u] = *reinterpret_cast<const Raw *>(tab + ea.x * stride + (eb.y * K + in_slot));
        y[u] = *reinterpret_cast<const Raw *>(tab + eb.x * stride + (ea.y * K + in_slot));
        if (q + PPS < n_pairs) cur.advance(PPS, nv);
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        float4 xf[VPL], yf[VPL];
        serve8_widen(x[u], sa[u], xf);
        serve8_widen(y[u], sb[u], yf);
        const float term = wave_pair_term<LPP, VPL>(xf, yf, c, xa[u], xb[u]);
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

// ---- the encoder ---------------------------------------------------------------------------------------

// s of a row whose largest finite |w| has the bits `abits` (0: no finite nonzero element, scale 1.0f).
__device__ __forceinline__ int serve8_scale_exp(unsigned abits) {
  if (abits == 0u) return 0;
  const int e = static_cast<int>(abits >> 23);  // (a subnormal A clamps to -117)
  int s = e == 0 ? -117 : min(max(e - 127 - 8, -117), 119);
  if (__uint_as_float(abits) * __uint_as_float(static_cast<unsigned>(127 - s) << 23) > 448.0f) s++;
  return s;
}
__device__ __forceinline__ float serve8_pow2(int s) { return __uint_as_float(static_cast<unsigned>(127 + s) << 23); }

__device__ __forceinline__ unsigned serve8_absmax(float4 w, unsigned a) {
  const unsigned bits[4] = {__float_as_uint(w.x), __float_as_uint(w.y), __float_as_uint(w.z), __float_as_uint(w.w)};
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const unsigned ab = bits[c] & 0x7fffffffu;
    if (ab < 0x7f800000u) a = max(a, ab);  // finite elements only
  }
  return a;
}

// Four elements -> four bytes.  inv = 2^-s: the products are exact (or far below the smallest subnormal),
// none exceeds 448, and the conversion rounds to nearest even.  A NaN or an infinity: the NaN byte, signed.
__device__ __forceinline__ unsigned serve8_enc4(float4 w, float inv) {
  int r = __builtin_amdgcn_cvt_pk_fp8_f32(w.x * inv, w.y * inv, 0, false);
  r = __builtin_amdgcn_cvt_pk_fp8_f32(w.z * inv, w.w * inv, r, true);
  unsigned q = static_cast<unsigned>(r);
  const unsigned bits[4] = {__float_as_uint(w.x), __float_as_uint(w.y), __float_as_uint(w.z), __float_as_uint(w.w)};
#pragma unroll
  for (int c = 0; c < 4; c++)
    if ((bits[c] & 0x7fffffffu) >= 0x7f800000u) q = (q & ~(0xffu << (8 * c))) | ((0x7fu | ((bits[c] >> 24) & 0x80u)) << (8 * c));
  return q;
}

// ffm_pack_stats' counters for four source elements and what their bytes decode to.
__device__ __forceinline__ void serve8_count4(float4 w, float4 d, unsigned (&part)[PK_COUNT]) {
  const float ws[4] = {w.x, w.y, w.z, w.w}, ds[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const unsigned wb = __float_as_uint(ws[c]), db = __float_as_uint(ds[c]);
    const bool nan = (wb & 0x7fffffffu) > 0x7f800000u, fin = (wb & 0x7fffffffu) < 0x7f800000u;
    part[PK_INEXACT] += (!nan && db != wb) ? 1u : 0u;
    part[PK_TO_INF] += (fin && (db & 0x7fffffffu) >= 0x7f800000u) ? 1u : 0u;
    part[PK_TO_ZERO] += (!nan && (wb & 0x7fffffffu) != 0u && (db & 0x7fffffffu) == 0u) ? 1u : 0u;
  }
  part[PK_LATENT] += 4u;
}

// Vectors 4 ch .. 4 ch + 3 of a row of RL4 vectors (row_len is a multiple of 4); beyond the row: zeros.
template <typename Load>
__device__ __forceinline__ void serve8_load_chunk(Load load, int ch, int RL4, float4 (&w)[4]) {
#pragma unroll
  for (int q = 0; q < 4; q++) w[q] = 4 * ch + q < RL4 ? load(4 * ch + q) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}
__device__ __forceinline__ void serve8_store_chunk(const float4 (&w)[4], int ch, int RL4, float inv, float scale, char *row,
                                                   unsigned (&part)[PK_COUNT]) {
  unsigned q[4];
#pragma unroll
  for (int v = 0; v < 4; v++) {
    q[v] = 0u;  // (padding bytes are zero)
    if (4 * ch + v < RL4) {
      q[v] = serve8_enc4(w[v], inv);
      serve8_count4(w[v], serve8_dec4(q[v], scale), part);
    }
  }
  *reinterpret_cast<uint4 *>(row + kServe8Head + 16 * ch) = make_uint4(q[0], q[1], q[2], q[3]);
}

// One feature row by a group of G lanes (gl: this lane's number in it; all G lanes call).  load(v): vector v
// of the row's fp32 source; row: the row's first byte in the table.
template <int G, typename Load>
__device__ __forceinline__ void serve8_encode_row(Load load, char *row, int row_len, int gl, unsigned (&part)[PK_COUNT]) {
  static_assert(G == 16 || G == 64, "a quarter of a wave for short rows, or a whole one");
  const int RL4 = row_len >> 2, n_ch = (row_len + 15) >> 4;
  float4 kept[4];  // the lane's first chunk stays in registers
  unsigned a = 0u;
  if (gl < n_ch) {
    serve8_load_chunk(load, gl, RL4, kept);
#pragma unroll
    for (int v = 0; v < 4; v++) a = serve8_absmax(kept[v], a);
  }
  for (int ch = gl + G; ch < n_ch; ch += G) {
    float4 w[4];
    serve8_load_chunk(load, ch, RL4, w);
#pragma unroll
    for (int v = 0; v < 4; v++) a = serve8_absmax(w[v], a);
  }
#pragma unroll
  for (int d = G / 2; d >= 1; d >>= 1) a = max(a, static_cast<unsigned>(__shfl_xor(static_cast<int>(a), d, 64)));
  const int s = serve8_scale_exp(a);
  const float inv = serve8_pow2(-s), scale = serve8_pow2(s);
  if (gl == 0) *reinterpret_cast<uint4 *>(row) = make_uint4(__float_as_uint(scale), 0u, 0u, 0u);
  if (gl < n_ch) serve8_store_chunk(kept, gl, RL4, inv, scale, row, part);
  for (int ch = gl + G; ch < n_ch; ch += G) {  // (the second read of a long row)
    float4 w[4];
    serve8_load_chunk(load, ch, RL4, w);
    serve8_store_chunk(w, ch, RL4, inv, scale, row, part);
  }
}

constexpr int kServe8Threads = 256;
// Lanes per row for a row length: a quarter wave while it keeps the row in registers.
inline int serve8_group(int row_len) { return row_len <= 16 * 16 ? 16 : 64; }

__device__ __forceinline__ void serve8_counters_out(const unsigned (&part)[PK_COUNT], unsigned long long *counters) {
#pragma unroll
  for (int k = 0; k < PK_COUNT; k++) {
    const unsigned long long sum = serve_wave_sum(part[k]);
    if ((threadIdx.x & 63) == 0 && sum != 0ull)
      __hip_atomic_fetch_add(counters + k * kPackLine, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ffm_engine_pack_weights on an f8 engine: src's stored bias, lin_w and the w of every record, counted as
// serve_pack_kernel counts (one atomic per counter and wave).
template <int G>
__global__ __launch_bounds__(kServe8Threads) FFM_SERVE8_FN void serve_pack8_kernel(ModelDev src, ModelDev dst, unsigned long long *counters) {
  const int64_t T = static_cast<int64_t>(gridDim.x) * kServe8Threads;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kServe8Threads + threadIdx.x;
  for (int64_t i = t; i < src.n_feats; i += T) dst.lin_w[i] = __builtin_nontemporal_load(src.lin_w + i);
  if (t == 0) dst.bias3[0] = src.bias3[0];
  const int64_t RL4 = src.row_len / 4, stride = serve8_stride(dst.row_len);
  const float4 *const rec = reinterpret_cast<const float4 *>(src.lat);
  char *const tab = reinterpret_cast<char *>(dst.lat);
  unsigned part[PK_COUNT] = {0u, 0u, 0u, 0u};
  const int gl = threadIdx.x % G;
  for (int64_t f = t / G; f < src.n_feats; f += T / G) {
    const float4 *const w = rec + f * 3 * RL4 + LAT_W * RL4;
    serve8_encode_row<G>([&](int v) { return load_nt(w + v); }, tab + f * stride, dst.row_len, gl, part);
  }
  serve8_counters_out(part, counters);
}

// Create-time contents: the elements a training engine would draw (same seed, same index), encoded row by
// row; zero != 0: rows of zeros (FFM_FLAG_SKIP_INIT -- every row still gets its head, scale 1.0f).  Nobody reads
// the counters of a draw: `part` is dead here and the compiler drops its arithmetic.
template <int G>
__global__ __launch_bounds__(kServe8Threads) FFM_SERVE8_FN void serve8_init_kernel(ModelDev m, float mean, float stddev, uint64_t seed, int zero) {
  const int64_t T = static_cast<int64_t>(gridDim.x) * kServe8Threads;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kServe8Threads + threadIdx.x;
  if (!zero)
    for (int64_t i = t; i < m.n_feats; i += T) m.lin_w[i] = ftrl_rng::init_weight(seed, 0, i, mean, stddev);
  const int64_t stride = serve8_stride(m.row_len);
  char *const tab = reinterpret_cast<char *>(m.lat);
  unsigned part[PK_COUNT] = {0u, 0u, 0u, 0u};
  const int gl = threadIdx.x % G;
  for (int64_t f = t / G; f < m.n_feats; f += T / G) {
    const int64_t first = f * m.row_len;
    serve8_encode_row<G>(
        [&](int v) {
          if (zero) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
          const int64_t idx = first + 4 * v;
          return make_float4(ftrl_rng::init_weight(seed, 1, idx, mean, stddev), ftrl_rng::init_weight(seed, 1, idx + 1, mean, stddev),
                             ftrl_rng::init_weight(seed, 1, idx + 2, mean, stddev), ftrl_rng::init_weight(seed, 1, idx + 3, mean, stddev));
        },
        tab + f * stride, m.row_len, gl, part);
  }
}

// dense[j][row_len] fp32 -> the rows of features ids[j] (ids == NULL: feat0 + j), whole rows, each with the
// scale of the values given, counted into `counters` as serve_pack8_kernel counts (ffm_engine_encode_stats).  An
// id outside the table is skipped (the engine checked the list).
template <int G>
__global__ __launch_bounds__(kServe8Threads) FFM_SERVE8_FN void serve8_encode_kernel(ModelDev m, const float *dense, const int *ids, int64_t feat0,
                                                                                     int64_t nf, unsigned long long *counters) {
  const int64_t T = static_cast<int64_t>(gridDim.x) * kServe8Threads;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kServe8Threads + threadIdx.x;
  const int64_t RL4 = m.row_len / 4, stride = serve8_stride(m.row_len);
  char *const tab = reinterpret_cast<char *>(m.lat);
  unsigned part[PK_COUNT] = {0u, 0u, 0u, 0u};
  const int gl = threadIdx.x % G;
  for (int64_t j = t / G; j < nf; j += T / G) {
    const int64_t f = ids ? static_cast<int64_t>(ids[j]) : feat0 + j;
    if (f < 0 || f >= m.n_feats) continue;  // (uniform across the row's group)
    const float4 *const w = reinterpret_cast<const float4 *>(dense) + j * RL4;
    serve8_encode_row<G>([&](int v) { return w[v]; }, tab + f * stride, m.row_len, gl, part);
  }
  serve8_counters_out(part, counters);
}

// The rows of features ids[j] (ids == NULL: feat0 + j) -> dense[j][row_len] fp32, four elements per thread;
// an id outside the table reads as zeros.
__global__ FFM_SERVE8_FN void serve8_decode_kernel(ModelDev m, float *dense, const int *ids, int64_t feat0, int64_t nf) {
  const int64_t RL4 = m.row_len / 4, total = nf * RL4, stride = serve8_stride(m.row_len);
  const int64_t T = static_cast<int64_t>(gridDim.x) * blockDim.x;
  const char *const tab = reinterpret_cast<const char *>(m.lat);
  for (int64_t it = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; it < total; it += T) {
    const int64_t j = it / RL4, v = it - j * RL4;
    const int64_t f = ids ? static_cast<int64_t>(ids[j]) : feat0 + j;
    float4 w = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (f >= 0 && f < m.n_feats) {
      const char *const row = tab + f * stride;
      w = serve8_dec4(*reinterpret_cast<const unsigned *>(row + kServe8Head + 4 * v), *reinterpret_cast<const float *>(row));
    }
    reinterpret_cast<float4 *>(dense)[it] = w;
  }
}

}  // namespace ftrl_dev
