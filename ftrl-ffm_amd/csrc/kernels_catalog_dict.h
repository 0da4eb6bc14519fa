// kernels_catalog_dict.h -- the FACTORISED item table (include/ffm_engine.h "Scoring a catalogue: dictionary slots"):
// kernels_catalog_items.h's items whose last n_dict slots hold, instead of a model id, a CODE into a small dictionary
// of their own -- advertiser, category, size: a thousand, a hundred, ten ids under millions of items.  A slot's
// contribution sum_j U_r^a[j] W[c_a][j] depends on the request and the slot's id alone, so it is computed once per
// DISTINCT id and added per item by lookup; only the first n_gather slots go through the gathered contraction.
//   score(r, c) = base_r + S_c + sum_{a < n_gather} sum_j U_r^a[j] W[c_a][j] + sum_{a' < n_dict} P_a'[code_a'(c)][r]
//   P_a'[d][r]  = sum_j U_r^a[j] W[dict_a'[d]][j]                     a = n_gather + a', rounded to fp32 once
//
//   catalog_dict_u_kernel<FMT>          one wave per (dictionary slot, request): U_r^a, v_a folded in, as a block
//                                       [rows][Lp] of its own -- on f16 its own two planes and its own shift per
//                                       (slot, request) -- so every slot is a complete CatalogDev (catalog_dict_slot_dev)
//   catalog_dict_kernel<FMT, RT>        one launch over all dictionaries laid end to end, each padded to whole waves
//                                       of 32 columns: catalog_accumulate over CatalogItemSrc with ONE slot, the
//                                       wave's slot; writes P request-minor
//   catalog_dict_self_kernel<FMT>       catalog_items_self_kernel with the dictionary slots' ids read through
//                                       their dictionaries (catalog_items_self_sum adds them: pairs between two
//                                       dictionary slots included, per item)
//   catalog_dict_gemm_kernel            catalog_gemm_kernel<FMT, RT, CatalogDictSrc>
//   catalog_dict_topk_kernel            catalog_topk_kernel<FMT, RT, CatalogDictSrc>
// (the last two names are the profile calls' labels; the kernels are instantiations of the one text)
//
// P  fp32 [columns][rows], rows the call's padded request count: column dd.col[a'] + d is entry d of dictionary a'.
// A wave's 32 columns lie in one dictionary (every dictionary starts at a multiple of 32), so its slot, that slot's
// CatalogDev and its dictionary's base are wave-uniform, found by a chain of selects over dd.col.  The wave parks its
// 32 ids as CatalogItemSrc parks one slot's -- the source is used as it stands, with the dictionary as a one-slot
// item table -- and a lane's accumulators x = 4 q .. 4 q + 3 are four consecutive requests of ONE column: un-shifted
// (f16: by the slot's own shift of each request) they go out as one 16-byte store, 4 RT per lane.  Columns of the
// padding and of an id outside [0, n_feats) hold +0.0 (written, not computed).  128 requests x 1 110 ids are 0.57 MB:
// P lives in L2 for the item kernels; it is not staged in LDS.
//
// THE DICTIONARY SOURCE (CatalogDictSrc)  CatalogItemSrc over the n_gather gathered slots, and a Term (kernels_catalog.h
// "ROW SOURCES") that adds the dictionary slots behind the accumulation.  A lane reads its column's n_dict codes once
// (per slab in the top-K kernel) and keeps dd.col[a'] + code, or -1 for a code outside [0, D_a') and for a column
// beyond the table.  Per tile and slot it then reads four 16-byte vectors P[col][r_tile + 8 q + 4 h ..] -- 4 RT loads
// per slot where a request-major P would take 16 RT scattered words -- and a slot of -1 adds +0.0 without a load.
// ORDER, fixed, the same function in the matrix and the top-K kernel, so a (request, item) pair has the same bits
// from both:
//   t = acc'                        the gathered slots' accumulator, un-shifted on f16 (the gathered slots' one shift)
//   t = fadd(t, P_a')               a' = 0 .. n_dict - 1, in slot order
//   score = fadd(t, fadd(S_c, base_r))
//
// NOT BIT FOR BIT against score_items or the rows.  For finite tables the bound of kernels_catalog_items.h carries
// over unchanged, with m = n_gather + n_dict and N = m L + m + m (m - 1) / 2 k:
//   |score - (base_r + ref64)| <= (N + 32) * 2^-24 * (|base_r| + scale)     (score_items_reference on expand_items(...))
// The N products are the same; each P_a' is the fp32 sum of its slot's L products in the matrix unit's order, rounded
// once, and the partial sums are added in slot order: one more summation order of the same N products, which the
// any-order term N * 2^-24 covers.  On f16 every dictionary slot has a shift of its own per request, chosen from its
// own block's largest magnitude: at least as tight as the one shift over all blocks that the 32 covers there.
//
// RESOURCES (hipcc --offload-arch=gfx950 -O3, kernel-resource-usage; no scratch in any of them; static LDS of the
// dict, gemm and top-K instantiations 38 912 bytes)
//   catalog_dict_u_kernel<f32>       16 VGPRs, 8 waves     <f16>  18 VGPRs, 8 waves
//   catalog_dict_self_kernel<f32>    38 VGPRs, 8 waves     <f16>  32 VGPRs, 8 waves      catalog_dict_fields_kernel  12 VGPRs
//   catalog_dict_kernel (VGPRs, AGPRs, waves per SIMD)
//         <f32, 1>   60, 16, 4      <f32, 2>   62, 32, 4      <f32, 4>   86, 64, 3
//         <f16, 1>   66, 16, 4      <f16, 2>   82, 32, 4      <f16, 4>  112, 64, 2
//   gemm  <f32, 1>   62, 16, 4      <f32, 2>   70, 32, 4      <f32, 4>  102, 64, 3
//         <f16, 1>   68, 16, 4      <f16, 2>   90, 32, 4      <f16, 4>  122, 64, 2
//   topk  <f32, 1>   92, 16, 4      <f32, 2>  110, 32, 3      <f32, 4>  166, 64, 2
//         <f16, 1>   96, 16, 4      <f16, 2>  110, 32, 3      <f16, 4>  168, 64, 2
// The 24 instantiations over CatalogSlabSrc and CatalogItemSrc keep, register for register, the counts of their
// headers: their Term is CatalogNoTerm, which holds and does nothing.  (catalog_items_self_kernel<f32> went from 44 to
// 38 VGPRs when its sums moved into catalog_items_self_sum; the operations and their order are what they were.)
#pragma once
#include "kernels_catalog_items.h"

namespace ftrl_dev {

// The dictionaries of a call, by value into the kernels.  Dictionary a' has the entries [ptr[a'], ptr[a' + 1]) of
// dict_feat and the columns [col[a'], col[a' + 1]) of P, its size rounded up to whole waves of 32.
struct CatalogDicts {
  int n;  // n_dict, in [1, kItemSlots - 1]
  int ptr[kItemSlots];
  int col[kItemSlots];
};

// Dictionary slot a of the blocks cd0 describes (cd0.u, cd0.shift: slot 0's; every slot [rows][lp], the shifts [rows]).
__device__ __forceinline__ CatalogDev catalog_dict_slot_dev(const CatalogDev &cd0, int a) {
  CatalogDev cd = cd0;
  cd.u = static_cast<char *>(cd0.u) + static_cast<int64_t>(a) * cd0.rows * cd0.lp * 4;  // (fp32, or two planes of halves)
  cd.shift = cd0.shift + static_cast<int64_t>(a) * cd0.rows;
  return cd;
}

// field[p] = the field of entry p of dict_feat, for the host calls' hashing; sl: the dictionary slots alone.
__global__ __launch_bounds__(256) void catalog_dict_fields_kernel(CatalogItemSlots sl, CatalogDicts dd, int n, int *field) {
  for (int p = blockIdx.x * 256 + threadIdx.x; p < n; p += gridDim.x * 256) {
    int g = sl.field[0];
#pragma unroll
    for (int s = 1; s < kItemSlots - 1; s++) g = s < dd.n && p >= dd.ptr[s] ? sl.field[s] : g;
    field[p] = g;
  }
}

// One wave per (dictionary slot, request of the padded range): wave w is request w % rows of slot w / rows.
// sl: the dictionary slots alone; cd0: slot 0's block (catalog_dict_slot_dev).
template <int FMT>
__global__ __launch_bounds__(64 * kPredRows) void catalog_dict_u_kernel(ModelDev m, int n_req, const int *ctx_ptr, const int *field,
                                                                       const int *feat, const float *val, CatalogItemSlots sl,
                                                                       CatalogDev cd0, int max_row_nnz, int lds_cap) {
  static_assert(FMT == SERVE_F32 || FMT == SERVE_F16, "a packed table of w alone");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int w = wave_uniform(blockIdx.x * kPredRows + wv);
  if (w >= cd0.rows * sl.n) return;
  const int a = w / cd0.rows, r = w - a * cd0.rows;
  int g = sl.field[0];
  float v = sl.val[0];
#pragma unroll
  for (int s = 1; s < kItemSlots - 1; s++) {
    g = a == s ? sl.field[s] : g;
    v = a == s ? sl.val[s] : v;
  }
  int4 *const E = wave_lds(smem, wv, lds_cap, 0).E;
  int nv = 0;
  catalog_stage_context(m, r, n_req, ctx_ptr, field, feat, val, max_row_nnz, lds_cap, lane, E, nv);
  catalog_u_store<FMT>([&](int j) { return __fmul_rn(v, catalog_u_element<FMT>(m, E, nv, g, j)); }, m.row_len,
                       catalog_dict_slot_dev(cd0, a), r, lane);
}

// Requests [r0, r0 + 32 RT) (rows of cd0, whole tiles, all of them stored: U is zero from n_req on) against the
// columns [128 blockIdx.x, ...) of all dictionaries; tab: row 0 of the table; P [dd.col[dd.n]][cd0.rows].
template <int FMT, int RT>
__global__ __launch_bounds__(64 * kCatWaves) void catalog_dict_kernel(const char *tab, int L, CatalogDev cd0, int r0, CatalogDicts dd,
                                                                     const int *dict_feat, int n_feats, float *P) {
  static_assert(FMT == SERVE_F32 || FMT == SERVE_F16, "a packed table of w alone");
  static_assert(RT == 1 || RT == 2 || RT == 4, "request tiles per launch");
  constexpr int ES = FMT == SERVE_F16 ? 2 : 4;
  __shared__ __attribute__((aligned(16))) char tile[kCatWaves][32 * kCatRowBytes];
  __shared__ int own[kCatWaves][CatalogItemSrc::kLdsInts];
  const int lane = threadIdx.x & 63, wv = wave_uniform(static_cast<int>(threadIdx.x >> 6));
  const int col0 = (blockIdx.x * kCatWaves + wv) * 32;  // the wave's first column
  // (dd.col[dd.n]: all columns; dd.n <= kItemSlots - 1)
  int a = 0, base = 0, first = dd.ptr[0], end = dd.ptr[1], total = dd.col[1];
#pragma unroll
  for (int s = 1; s < kItemSlots - 1; s++) {
    const bool in = s < dd.n && col0 >= dd.col[s];
    a = in ? s : a;
    base = in ? dd.col[s] : base;
    first = in ? dd.ptr[s] : first;
    end = in ? dd.ptr[s + 1] : end;
    total = s < dd.n ? dd.col[s + 1] : total;
  }
  if (col0 >= total) return;  // (nothing below waits for another wave)
  const int64_t c0 = col0 - base, n_ids = end - first;  // the wave's first entry of its dictionary, and the dictionary's size
  const CatalogDev cd = catalog_dict_slot_dev(cd0, a);
  const CatalogItemSrc::Args one{dict_feat + first, n_feats, 1, cd.lp * ES / kCatChunkBytes};
  const int j = lane & 31, h = lane >> 5;
  cat_v16f acc[RT];
  catalog_accumulate<FMT, RT>(tab, L, cd, r0, c0, n_ids, tile[wv], lane, acc, CatalogItemSrc(one, own[wv], c0, n_ids, lane));

  // ---- accumulators 4 q .. 4 q + 3 of a lane: requests 8 q + 4 h .. + 3 of the tile, column lane % 32
  const bool erased = own[wv][j] == n_feats;  // the padding, an id outside the table (behind catalog_accumulate's closing fence)
  float *const out = P + static_cast<int64_t>(col0 + j) * cd.rows;
#pragma unroll
  for (int t = 0; t < RT; t++)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int r = r0 + kCatTile * t + 8 * q + 4 * h;
      float4 p = make_float4(acc[t][4 * q], acc[t][4 * q + 1], acc[t][4 * q + 2], acc[t][4 * q + 3]);
      if (FMT == SERVE_F16) {
        const int4 s = *reinterpret_cast<const int4 *>(cd.shift + r);
        p = make_float4(ldexpf(p.x, -s.x), ldexpf(p.y, -s.y), ldexpf(p.z, -s.z), ldexpf(p.w, -s.w));
      }
      *reinterpret_cast<float4 *>(out + r) = erased ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : p;
    }
}

// S_c of every item: catalog_items_self_kernel's lanes and sums; sl: all slots, the n_gather gathered ones first.
template <int FMT>
__global__ __launch_bounds__(256) void catalog_dict_self_kernel(ModelDev m, CatalogItemSlots sl, int n_gather, const int *item_feat,
                                                                const int *item_code, CatalogDicts dd, const int *dict_feat,
                                                                int64_t n_items, float *item_s) {
  static_assert(FMT == SERVE_F32 || FMT == SERVE_F16, "a packed table of w alone");
  const int64_t c = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 2;
  const int q = threadIdx.x & 3;
  const bool live = c < n_items;
  int id[kItemSlots];
#pragma unroll
  for (int a = 0; a < kItemSlots; a++) {
    id[a] = -1;
    if (!live || a >= sl.n) continue;
    int i = -1;
    if (a < n_gather) i = item_feat[c * n_gather + a];
    else {
      // (slot a is dictionary a - n_gather: its bounds by selects, dd lives in scalar registers)
      int first = dd.ptr[0], end = dd.ptr[1];
#pragma unroll
      for (int s = 1; s < kItemSlots - 1; s++) {
        first = a - n_gather == s ? dd.ptr[s] : first;
        end = a - n_gather == s ? dd.ptr[s + 1] : end;
      }
      const int code = item_code[c * dd.n + (a - n_gather)];
      if (code >= 0 && code < end - first) i = dict_feat[first + code];
    }
    id[a] = i >= 0 && i < m.n_feats ? i : -1;
  }
  const float sum = catalog_items_self_sum<FMT>(m, sl, id, q);
  if (live && q == 0) item_s[c] = sum;
}

// The dictionary source of the two kernels.  Their common arguments mean what they mean over CatalogItemSrc.
struct CatalogDictSrc : CatalogItemSrc {
  struct Args {
    CatalogItemSrc::Args items;  // the gathered slots: item_feat [n_items][n_gather]
    const int *item_code;        // [n_items][dd.n]
    const float *P;              // [dd.col[dd.n]][rows]
    CatalogDicts dd;
    int rows;
  };
  __device__ __forceinline__ CatalogDictSrc(const Args &t, int *lds, int64_t c0, int64_t n_items, int lane)
      : CatalogItemSrc(t.items, lds, c0, n_items, lane) {}
  struct Term {
    const float *P;
    int rows, n;
    int col[kItemSlots - 1];  // of P, per dictionary slot; -1: adds +0.0
    __device__ __forceinline__ Term(const Args &t, int64_t c, int64_t n_items) : P(t.P), rows(t.rows), n(t.dd.n) {
#pragma unroll
      for (int s = 0; s < kItemSlots - 1; s++) {
        col[s] = -1;
        if (s < t.dd.n && c < n_items) {
          const int code = t.item_code[c * t.dd.n + s];
          if (code >= 0 && code < t.dd.ptr[s + 1] - t.dd.ptr[s]) col[s] = t.dd.col[s] + code;
        }
      }
    }
    // a: the lane's accumulators of the tile whose first request is r_tile (a row of P's padded range); shift: the
    // tile's 32 shifts (f16).  Afterwards a holds t of ORDER above: logit adds the rest and does not shift again.
    template <int FMT>
    __device__ __forceinline__ void add(cat_v16f &a, int r_tile, int h, const int *shift) const {
      if (FMT == SERVE_F16) {
#pragma unroll
        for (int x = 0; x < 16; x++) a[x] = ldexpf(a[x], -shift[8 * (x >> 2) + 4 * h + (x & 3)]);
      }
#pragma unroll
      for (int s = 0; s < kItemSlots - 1; s++) {
        if (s >= n) break;  // (wave-uniform)
        float4 p[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
          p[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
          if (col[s] >= 0) p[q] = *reinterpret_cast<const float4 *>(P + static_cast<int64_t>(col[s]) * rows + r_tile + 8 * q + 4 * h);
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
          a[4 * q] = __fadd_rn(a[4 * q], p[q].x);
          a[4 * q + 1] = __fadd_rn(a[4 * q + 1], p[q].y);
          a[4 * q + 2] = __fadd_rn(a[4 * q + 2], p[q].z);
          a[4 * q + 3] = __fadd_rn(a[4 * q + 3], p[q].w);
        }
      }
    }
  };
  template <int FMT>
  static __device__ __forceinline__ float logit(float a, float, float s, float base, int) {
    return __fadd_rn(a, __fadd_rn(s, base));
  }
};

}  // namespace ftrl_dev
