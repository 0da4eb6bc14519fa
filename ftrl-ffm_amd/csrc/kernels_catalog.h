// kernels_catalog.h -- request contexts against a whole id range of one field (include/ffm_engine.h "Scoring a
// catalogue").  A candidate is the single entry (g, c, v), c in [cand_first, cand_first + n_cand), and
//   score(r, c) = base_r + v * lin_w[c] + v * sum_{j < L} U_r[j] * W[c][j]          L = n_fields * n_factors
// with W[c] candidate c's whole serving-table row, U_r[f * k + t] the sum over the context's entries i of field f,
// in entry order, of fl(val_i * w[id_i][g * k + t]), and base_r the row kernel's logit of the context alone.  The
// pair sum of every request and candidate is therefore out[R][C] = U[R][L] * W[C][L]^T over a CONTIGUOUS slab of
// the table: a dense contraction of length L (624 at 39 fields x 16 factors), streamed, not gathered -- the one
// place in this project where the matrix unit fits.
//
//   catalog_u_kernel<FMT>         one wave per request: U_r, zero-filled to Lp (whole chunks) and to whole request tiles
//   catalog_gemm_kernel<FMT, RT>  four waves own a run of 128 candidates, 32 each, against RT tiles of 32 requests
//
// NOT BIT FOR BIT: the sum over j runs in the matrix unit's order.  For finite tables
//   |score - (base_r + dot64)| <= (L + 32) * 2^-24 * (|base_r| + scale)
// with dot64 and scale from score_catalog_reference (engine.py): L * 2^-24 is the any-order bound of an fp32 sum of
// L products; the other 32 * 2^-24 covers U's own fp32 sums (contexts of a few entries per field), the two fp16
// planes of U on an f16 engine (at most 2^-21 max|U| per element, below) and the epilogue's two fused roundings.
//
// OPERANDS  A chunk is 256 bytes of a candidate's row: 64 floats or 128 halves.  Both formats move through the same
// path: a lane's 16-byte vector is one k-block of its row, and the k-order inside the matrix instruction is the same
// function of (lane / 32, element) for A and B, so which k a slot stands for never matters as long as U is read by
// the rule W is read by.
//   B (the table)  each wave brings its 32 rows of the chunk in with 8 loads of 16 bytes per lane, 16 consecutive
//     lanes on the 256 consecutive bytes of one row (four rows per instruction), prefetched into registers one chunk
//     ahead, and hands them to the MFMA layout through its own LDS tile [32][256 + 16 pad] bytes: lane (j = lane % 32,
//     h = lane / 32) reads 16 bytes at row j, byte 32 q + 16 h of step q -- 272-byte rows put 16 lanes' vectors on
//     all 64 banks.  The tile is the wave's alone: no workgroup barrier anywhere.  A row is read from HBM once per
//     launch and its fragment reused across the RT request tiles.  The table's halves go in as they are stored.
//   A (U)  read per step from global memory (at most 128 * Lp * 4 bytes per launch: cache resident), 16 bytes per
//     lane at row i = lane % 32 of the tile, the same byte offset as B.
//   f32  __builtin_amdgcn_mfma_f32_32x32x2f32, four per step (the vector's four floats), both operands exact.
//   f16  __builtin_amdgcn_mfma_f32_32x32x16_f16, two per step: U's `hi` plane and its `lo` plane into the same
//     accumulators.  hi + lo ~= U * 2^s, s per request the power of two that puts max |U_r| into [2^13, 2^14) (0 for
//     an all-zero or non-finite U): hi = rn16(U 2^s), lo = rn16(U 2^s - hi), so |U 2^s - hi - lo| <= 4 * 2^-11 =
//     2^-22 max, and nothing of U rides on how the unit treats fp16 subnormals.  Un-scaled in the epilogue.
//   Tails: U is zero beyond L and beyond n_req; table vectors beyond the row's bytes or beyond the last candidate are
//     zero registers, never loads; stores are guarded.  out is indexed in 64 bits.
//   Epilogue: fma(v, acc, fma(v, lin_w[c], base_r)), sigmoid_ref under output_prob.  v == 0 gives base_r itself.
//
// RESOURCES (hipcc --offload-arch=gfx950 -O3, kernel-resource-usage; no scratch in any of them; the gemm's 34 816
// bytes of LDS per workgroup allow four workgroups = four waves per SIMD, so registers bind only where noted)
//   catalog_u_kernel<f32 | f16>    16 VGPRs, 0 AGPRs, 8 waves per SIMD
//   catalog_gemm_kernel<f32, 1>    78 VGPRs, 16 AGPRs, 4 waves      <f16, 1>   84 VGPRs, 16 AGPRs, 4 waves
//   catalog_gemm_kernel<f32, 2>    92 VGPRs, 32 AGPRs, 4 waves      <f16, 2>  100 VGPRs, 32 AGPRs, 3 waves (registers)
//   catalog_gemm_kernel<f32, 4>   104 VGPRs, 64 AGPRs, 3 waves (registers)   <f16, 4>  130 VGPRs, 64 AGPRs, 2 waves (registers)
#pragma once
#include <hip/hip_fp16.h>

#include "engine_types.h"
#include "kernels_wave.h"

namespace ftrl_dev {

constexpr int kCatChunkBytes = 256;                // of a candidate's row per chunk
constexpr int kCatRowBytes = kCatChunkBytes + 16;  // ... in LDS
constexpr int kCatWaves = 4, kCatCands = 32 * kCatWaves;
constexpr int kCatTile = 32;  // requests per tile

__host__ __device__ inline int catalog_chunk_elems(int fmt) { return kCatChunkBytes / (fmt == SERVE_F16 ? 2 : 4); }
// L in whole chunks: the row length of U
__host__ __device__ inline int catalog_lp(int fmt, int L) {
  const int c = catalog_chunk_elems(fmt);
  return (L + c - 1) / c * c;
}

// What catalog_u_kernel leaves for catalog_gemm_kernel.  rows: the requests in whole tiles of the launches.
struct CatalogDev {
  float *base;  // [rows] the context's own logit (the row kernel's)
  void *u;      // f32: float [rows][Lp]; f16: two planes of halves [rows][Lp], hi then lo
  int *shift;   // [rows] s of the request (f16; 0 on an f32 engine)
  int rows, lp;
};

typedef _Float16 cat_v8h __attribute__((ext_vector_type(8)));
typedef float cat_v16f __attribute__((ext_vector_type(16)));

// What a wave writes of its request r: element(j) for j < cd.lp (0 from the live length on) as U's row, on f16 as the
// two planes under the request's one shift.  n_scan: the elements the largest magnitude is looked for among (the rest
// are zero).
template <int FMT, typename Element>
__device__ __forceinline__ void catalog_u_store(Element element, int n_scan, const CatalogDev &cd, int r, int lane) {
  const int64_t row = static_cast<int64_t>(r) * cd.lp;
  if (FMT == SERVE_F32) {
    float *const U = static_cast<float *>(cd.u) + row;
    for (int j = lane; j < cd.lp; j += 64) U[j] = element(j);
    if (lane == 0) cd.shift[r] = 0;
    return;
  }
  // f16: the largest magnitude first, then the same sums again, scaled and split
  float big = 0.0f;
  bool odd = false;  // a NaN or an infinity
  for (int j = lane; j < n_scan; j += 64) {
    const float u = fabsf(element(j));
    odd = odd || !(u <= 3.4028234664e38f);
    big = fmaxf(big, u);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) big = fmaxf(big, __shfl_xor(big, d, 64));
  int s = 0;
  if (__ballot(odd) == 0ull && big > 0.0f) {
    int ex;
    (void)frexpf(big, &ex);  // big = fr * 2^ex, fr in [0.5, 1)
    s = 14 - ex;
  }
  __half *const hi = static_cast<__half *>(cd.u) + row, *const lo = hi + static_cast<int64_t>(cd.rows) * cd.lp;
  for (int j = lane; j < cd.lp; j += 64) {
    const float x = ldexpf(element(j), s);
    const __half h = __float2half_rn(x);
    hi[j] = h;
    lo[j] = __float2half_rn(__fsub_rn(x, __half2float(h)));
  }
  if (lane == 0) cd.shift[r] = s;
}

// The context of request r into the wave's LDS (E; *nv survivors).  A context the row kernel refuses (longer than
// max_row_nnz or than a wave stages) and a row of the padding stage nothing: zeros in U, and the NaN comes from base.
__device__ __forceinline__ void catalog_stage_context(const ModelDev &m, int r, int n_req, const int *ctx_ptr, const int *field,
                                                      const int *feat, const float *val, int max_row_nnz, int lds_cap, int lane,
                                                      int4 *E, int &nv) {
  if (r >= n_req) return;
  const int b = wave_uniform(ctx_ptr[r]);
  const int nnz = wave_uniform(ctx_ptr[r + 1]) - b;
  if (nnz <= max_row_nnz && nnz <= lds_cap) {
    float unused = 0.0f;
    wave_stage_entries(m, feat, field, val, b, nnz, lane, unused, nv, [&](int at, int4 en, float) { E[at] = en; });
  }
}

// Element f * k + t of U_r towards field g: the staged entries of field f in order, each fl(val * w[id][g * k + t]).
template <int FMT>
__device__ __forceinline__ float catalog_u_element(const ModelDev &m, const int4 *E, int nv, int g, int j) {
  const int k = m.n_factors, L = m.row_len;
  float acc = 0.0f;
  if (j < L) {
    const int f = j / k, t = j - f * k;
    for (int p = 0; p < nv; p++) {
      const int4 en = E[p];
      if (en.y != f) continue;
      const int64_t at = static_cast<int64_t>(en.x) * L + g * k + t;
      const float w = FMT == SERVE_F16 ? serve_dec16(reinterpret_cast<const unsigned short *>(m.lat)[at]) : m.lat[at];
      acc = __fadd_rn(acc, __fmul_rn(__int_as_float(en.z), w));
    }
  }
  return acc;
}

// One wave per request of the padded range [0, cd.rows); kPredRows per workgroup.
template <int FMT>
__global__ __launch_bounds__(64 * kPredRows) void catalog_u_kernel(ModelDev m, int n_req, const int *ctx_ptr, const int *field,
                                                                  const int *feat, const float *val, int g, CatalogDev cd,
                                                                  int max_row_nnz, int lds_cap) {
  static_assert(FMT == SERVE_F32 || FMT == SERVE_F16, "a packed table of w alone");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = wave_uniform(blockIdx.x * kPredRows + wv);
  if (r >= cd.rows) return;
  int4 *const E = wave_lds(smem, wv, lds_cap, 0).E;
  int nv = 0;
  catalog_stage_context(m, r, n_req, ctx_ptr, field, feat, val, max_row_nnz, lds_cap, lane, E, nv);
  catalog_u_store<FMT>([&](int j) { return catalog_u_element<FMT>(m, E, nv, g, j); }, m.row_len, cd, r, lane);
}

// The wave's 16-byte vector of chunk `ch`: row `row4 + 4 it` of its 32, bytes [16 sub, 16 sub + 16) of the chunk.
// even16: the table's rows are whole 16-byte vectors (always on f32; on f16 when L % 8 == 0) -- otherwise rows are
// only 8-byte aligned and the vector comes as two halves, each inside the row or zero.
__device__ __forceinline__ uint4 catalog_load(const char *tab, int64_t row_bytes, int64_t cand, int64_t n_cand, int off, bool even16) {
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (cand >= n_cand) return v;
  const char *p = tab + cand * row_bytes + off;
  if (even16) {
    if (off + 16 <= row_bytes) v = *reinterpret_cast<const uint4 *>(p);
  } else {
    if (off + 8 <= row_bytes) {
      const uint2 a = *reinterpret_cast<const uint2 *>(p);
      v.x = a.x;
      v.y = a.y;
    }
    if (off + 16 <= row_bytes) {
      const uint2 b = *reinterpret_cast<const uint2 *>(p + 8);
      v.z = b.x;
      v.w = b.y;
    }
  }
  return v;
}

// ROW SOURCES  Where the B operand's rows come from is a policy of catalog_accumulate and of the two kernels: a slab of
// one field's ids (CatalogSlabSrc, here: stateless, so the slab's kernels are instruction for instruction what they
// were before there was a second source) or a table of items of several entries (kernels_catalog_items.h).  A source has
//   Args                  what its kernels take behind the common arguments (the slab: nothing)
//   kLdsInts              ints of LDS of its own per wave
//   Src(args, lds, c0, n_cols, lane)   made when the wave turns to the columns [c0, c0 + 32)
//   seek(ch)              chunk ch is the next to be loaded (chunks come in order from 0; wave-uniform)
//   load(tab, row_bytes, c0, row4, it, n_cols, ch, sub, even16)   16 bytes: row row4 + 4 it of the wave's 32, bytes
//                         [16 sub, 16 sub + 16) of chunk ch -- or zero registers where there is no such row or byte
//   logit<FMT>(a, v, col, base, shift)   the score of accumulator a; col: the column's own term (lin[c])
//   Term(args, c, n_cols)               made by a lane for its column c behind the accumulation (c may lie beyond n_cols)
//   term.add<FMT>(acc_t, r_tile, h, shift)   a term per (request, column) into the lane's 16 accumulators of the tile
//                         whose first request is r_tile, before logit sees them; shift: the tile's 32 shifts.
//                         CatalogNoTerm adds nothing and compiles to nothing (kernels_catalog_dict.h has the one that does)
// U's row has the chunks in the source's order: chunk ch pairs with bytes [256 ch, 256 ch + 256) of U_r.
struct CatalogNoTerm {
  template <typename Args>
  __device__ __forceinline__ CatalogNoTerm(const Args &, int64_t, int64_t) {}
  template <int FMT>
  __device__ __forceinline__ void add(cat_v16f &, int, int, const int *) const {}
};
struct CatalogSlabSrc {
  struct Args {};
  using Term = CatalogNoTerm;
  static constexpr int kLdsInts = 0;
  __device__ __forceinline__ CatalogSlabSrc() {}
  __device__ __forceinline__ CatalogSlabSrc(const Args &, int *, int64_t, int64_t, int) {}
  __device__ __forceinline__ void seek(int) {}
  __device__ __forceinline__ uint4 load(const char *tab, int64_t row_bytes, int64_t c0, int row4, int it, int64_t n_cand, int ch, int sub,
                                        bool even16) const {
    return catalog_load(tab, row_bytes, c0 + row4 + 4 * it, n_cand, ch * kCatChunkBytes + 16 * sub, even16);
  }
  template <int FMT>
  static __device__ __forceinline__ float logit(float a, float v, float lw, float base, int shift);  // (catalog_logit, below)
};

// The contraction of one wave: its 32 columns [c0, c0 + 32) against the RT request tiles from r0 on, every chunk of
// U's row through the wave's own tile T, one chunk prefetched.  acc[t][x] of a lane afterwards: request row
// 8 (x / 4) + 4 (lane / 32) + x % 4 of tile t, candidate lane % 32.  The sequence of matrix instructions of a tile
// does not depend on RT: catalog_gemm_kernel and catalog_topk_kernel (kernels_catalog_topk.h) both run this and no
// other, so a (request, candidate) pair gets the same accumulator bits from either, at any RT.
template <int FMT, int RT, typename Src = CatalogSlabSrc>
__device__ __forceinline__ void catalog_accumulate(const char *tab, int L, const CatalogDev &cd, int r0, int64_t c0, int64_t n_cand,
                                                   char *T, int lane, cat_v16f (&acc)[RT], Src src = Src()) {
  constexpr int ES = FMT == SERVE_F16 ? 2 : 4;
  const int64_t row_bytes = static_cast<int64_t>(L) * ES;
  const bool even16 = (row_bytes & 15) == 0;
  const int n_chunks = cd.lp * ES / kCatChunkBytes;
  const int row4 = lane >> 4, sub = lane & 15;  // the loads: four rows per instruction, 16 lanes along a row
  const int j = lane & 31, h = lane >> 5;       // the fragments: row j of the tile, k-block h of a step

#pragma unroll
  for (int t = 0; t < RT; t++)
#pragma unroll
    for (int x = 0; x < 16; x++) acc[t][x] = 0.0f;

  uint4 next[8];
  src.seek(0);
#pragma unroll
  for (int it = 0; it < 8; it++) next[it] = src.load(tab, row_bytes, c0, row4, it, n_cand, 0, sub, even16);

  const char *const U = static_cast<const char *>(cd.u);
  const int64_t u_row = static_cast<int64_t>(cd.lp) * ES, plane = static_cast<int64_t>(cd.rows) * u_row;
  for (int ch = 0; ch < n_chunks; ch++) {
#pragma unroll
    for (int it = 0; it < 8; it++) *reinterpret_cast<uint4 *>(T + (row4 + 4 * it) * kCatRowBytes + 16 * sub) = next[it];
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    if (ch + 1 < n_chunks) {
      src.seek(ch + 1);
#pragma unroll
      for (int it = 0; it < 8; it++) next[it] = src.load(tab, row_bytes, c0, row4, it, n_cand, ch + 1, sub, even16);
    }
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const int off = 32 * q + 16 * h;
      const uint4 braw = *reinterpret_cast<const uint4 *>(T + j * kCatRowBytes + off);
#pragma unroll
      for (int t = 0; t < RT; t++) {
        const char *const ua = U + (static_cast<int64_t>(r0 + kCatTile * t + j)) * u_row + ch * kCatChunkBytes + off;
        if constexpr (FMT == SERVE_F16) {
          const cat_v8h b = __builtin_bit_cast(cat_v8h, braw);
          const cat_v8h a_hi = *reinterpret_cast<const cat_v8h *>(ua), a_lo = *reinterpret_cast<const cat_v8h *>(ua + plane);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo, b, acc[t], 0, 0, 0);
        } else {
          const float4 a = *reinterpret_cast<const float4 *>(ua);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, __uint_as_float(braw.x), acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, __uint_as_float(braw.y), acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, __uint_as_float(braw.z), acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, __uint_as_float(braw.w), acc[t], 0, 0, 0);
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  }
}

// The epilogue of one accumulator, shared for the same reason: candidate value v, its linear weight lw, the request's
// base and (f16) shift.
template <int FMT>
__device__ __forceinline__ float catalog_logit(float a, float v, float lw, float base, int shift) {
  if (FMT == SERVE_F16) a = ldexpf(a, -shift);
  return __fmaf_rn(v, a, __fmaf_rn(v, lw, base));
}
template <int FMT>
__device__ __forceinline__ float CatalogSlabSrc::logit(float a, float v, float lw, float base, int shift) {
  return catalog_logit<FMT>(a, v, lw, base, shift);
}

// Requests [r0, r0 + 32 RT) (rows of cd, whole tiles; stores for r < n_req only) against candidates
// [128 blockIdx.x, ...) of the range's n_cand; tab: row 0 of the range (cand_first's), lin: its lin_w.  Over another row
// source (kernels_catalog_items.h) the columns are its n_cand items, tab the whole table, lin the items' own terms.
template <int FMT, int RT, typename Src = CatalogSlabSrc>
__global__ __launch_bounds__(64 * kCatWaves) void catalog_gemm_kernel(const char *tab, const float *lin, int L, CatalogDev cd, int r0,
                                                                     int n_req, int64_t n_cand, float v, int output_prob,
                                                                     float *out, typename Src::Args args) {
  static_assert(FMT == SERVE_F32 || FMT == SERVE_F16, "a packed table of w alone");
  static_assert(RT == 1 || RT == 2 || RT == 4, "request tiles per launch");
  __shared__ __attribute__((aligned(16))) char tile[kCatWaves][32 * kCatRowBytes];
  __shared__ int own[kCatWaves][Src::kLdsInts > 0 ? Src::kLdsInts : 1];  // (unused, and then not allocated, for the slab)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t c0 = static_cast<int64_t>(blockIdx.x) * kCatCands + wv * 32;  // the wave's first candidate
  if (c0 >= n_cand) return;  // (nothing below waits for another wave)
  const int j = lane & 31, h = lane >> 5;
  cat_v16f acc[RT];
  catalog_accumulate<FMT, RT>(tab, L, cd, r0, c0, n_cand, tile[wv], lane, acc, Src(args, own[wv], c0, n_cand, lane));

  // ---- accumulator x of a lane: request row 8 (x / 4) + 4 (lane / 32) + x % 4 of the tile, candidate lane % 32
  const int64_t c = c0 + j;
  if (c >= n_cand) return;
  const float lw = lin[c];
  const typename Src::Term term(args, c, n_cand);
#pragma unroll
  for (int t = 0; t < RT; t++) {
    term.template add<FMT>(acc[t], r0 + kCatTile * t, h, cd.shift + r0 + kCatTile * t);
#pragma unroll
    for (int x = 0; x < 16; x++) {
      const int r = r0 + kCatTile * t + 8 * (x >> 2) + 4 * h + (x & 3);
      if (r >= n_req) continue;
      const float score = Src::template logit<FMT>(acc[t][x], v, lw, cd.base[r], FMT == SERVE_F16 ? cd.shift[r] : 0);
      out[static_cast<int64_t>(r) * n_cand + c] = output_prob ? sigmoid_ref(score) : score;
    }
  }
}

}  // namespace ftrl_dev
