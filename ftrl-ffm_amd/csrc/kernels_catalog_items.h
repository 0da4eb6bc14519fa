// kernels_catalog_items.h -- request contexts against a table of ITEMS of several entries (include/ffm_engine.h
// "Scoring a catalogue: items of several entries"): kernels_catalog.h's contraction with a gathered B operand.  An
// item c is m <= 8 entries (g_a, c_a, v_a), a = 0 .. m - 1, in distinct fields g_a and with values v_a shared by all
// items, and
//   score(r, c) = base_r + S_c + sum_a sum_{j < L} U_r^a[j] * W[c_a][j]              L = n_fields * n_factors
//   U_r^a[f * k + t] = v_a * the sum over the context's entries i of field f, in entry order, of fl(val_i * w[id_i][g_a * k + t])
//   S_c = sum_a v_a lin_w[c_a] + sum_{a < b} v_a v_b sum_t w[c_a][g_b * k + t] * w[c_b][g_a * k + t]
// The pair sum of all requests and items is still one dense product, of length m * Lp: U's row is the m blocks U_r^a
// one behind the other (each zero-filled to Lp, whole chunks), and row c of the B operand is the m table rows
// W[c_0] .. W[c_{m-1}] one behind the other -- gathered whole, 256 bytes of one row per chunk, never copied.
//
//   catalog_items_u_kernel<FMT>         one wave per request: all m blocks of U_r, v_a folded in
//   catalog_items_self_kernel<FMT>      four lanes per item: S_c of every item, once per call
//   catalog_items_gemm_kernel           catalog_gemm_kernel<FMT, RT, CatalogItemSrc>: the one kernel text over the item source
//   catalog_items_topk_kernel           catalog_topk_kernel<FMT, RT, CatalogItemSrc> likewise (catalog_topk_merge_kernel
//                                       follows, cand_first = 0: an id is the item's index)
// (the two names are the profile calls' labels; the kernels are instantiations, not copies)
//
// THE ITEM SOURCE (CatalogItemSrc; kernels_catalog.h "ROW SOURCES")  Chunk ch of the m * Lp * ES / 256 belongs to slot
// a = ch / chunks_per_row and is bytes [256 (ch - a chunks_per_row), ...) of the row tab + id * row_bytes (64-bit),
// id = item_feat[c][a].  The wave parks the ids of its 32 items, slot-major [m][32], in 1 KB of LDS of its own when it
// turns to them (the source's constructor): an id outside [0, n_feats) and every slot of an item from n_items on are
// parked as n_feats -- a row beyond the table's last -- and load as zero registers, never from memory.  A load reads
// its row's id back from LDS (eight reads at immediate offsets from one address per chunk) instead of holding eight
// ids in registers across the matrix instructions: the slab's f32 RT 4 instantiation is 8 VGPRs from losing a wave.  The prefetch stays one chunk ahead across slot boundaries:
// seek() only moves (a, first chunk of a).  With 4 KB of ids the gemm's workgroup holds 38 912 bytes: four per CU still.
// ONE SHIFT per request on f16, over all m blocks: the slots share accumulators in the matrix unit.
// EPILOGUE  fadd(acc', fadd(S_c, base_r)), acc' un-shifted on f16 (catalog_items_logit: one function for both kernels).
// NOT BIT FOR BIT against rows; for finite tables, N = m L + m + m (m - 1) / 2 k,
//   |score - (base_r + ref64)| <= (N + 32) * 2^-24 * (|base_r| + scale)          (score_items_reference, engine.py)
//
// RESOURCES (hipcc --offload-arch=gfx950 -O3, kernel-resource-usage; no scratch in any of them; the static LDS of
// the gemm and top-K instantiations is 38 912 bytes; waves per SIMD as the registers admit them)
//   catalog_items_u_kernel<f32>      22 VGPRs, 8 waves     <f16>  21 VGPRs, 8 waves
//   catalog_items_self_kernel<f32>   38 VGPRs, 8 waves    <f16>  32 VGPRs, 8 waves      catalog_items_fields_kernel  28 VGPRs
//   gemm <f32, 1>   62 VGPRs, 16 AGPRs, 4 waves      <f16, 1>   68 VGPRs, 16 AGPRs, 4 waves
//   gemm <f32, 2>   64 VGPRs, 32 AGPRs, 4 waves      <f16, 2>   84 VGPRs, 32 AGPRs, 4 waves
//   gemm <f32, 4>   88 VGPRs, 64 AGPRs, 3 waves      <f16, 4>  114 VGPRs, 64 AGPRs, 2 waves
//   topk <f32, 1>   85 VGPRs, 16 AGPRs, 4 waves      <f16, 1>   91 VGPRs, 16 AGPRs, 4 waves
//   topk <f32, 2>  102 VGPRs, 32 AGPRs, 3 waves      <f16, 2>   90 VGPRs, 32 AGPRs, 4 waves
//   topk <f32, 4>  135 VGPRs, 64 AGPRs, 2 waves      <f16, 4>  133 VGPRs, 64 AGPRs, 2 waves
// The slab's twelve instantiations of the same two kernel texts keep, register for register, the counts of
// kernels_catalog.h and kernels_catalog_topk.h: their source is stateless, and the compiler sees what it saw.
// (the gemm's fewer VGPRs than the slab's: a gathered row's address is made per load from the parked id, where the
// slab's eight row addresses live in registers across the chunk loop)
#pragma once
#include "kernels_catalog.h"
#include "kernels_catalog_topk.h"

namespace ftrl_dev {

constexpr int kItemSlots = 8;  // entries of an item at the most

// The slots of an item table: what all items share.  By value into the kernels.
struct CatalogItemSlots {
  int n;                   // m
  int field[kItemSlots];   // distinct, in [0, n_fields)
  float val[kItemSlots];
};

// field[p] = the field of entry p of item_feat, for the host calls' hashing (engine_hash.h hashes entries under fields).
__global__ __launch_bounds__(256) void catalog_items_fields_kernel(CatalogItemSlots sl, int64_t n, int *field) {
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; p < n; p += static_cast<int64_t>(gridDim.x) * 256) {
    const int a = static_cast<int>(p % sl.n);
    int g = sl.field[0];
#pragma unroll
    for (int s = 1; s < kItemSlots; s++) g = a == s ? sl.field[s] : g;
    field[p] = g;
  }
}

// One wave per request of the padded range [0, cd.rows); kPredRows per workgroup.  cd.lp: m * Lp, the whole row.
template <int FMT>
__global__ __launch_bounds__(64 * kPredRows) void catalog_items_u_kernel(ModelDev m, int n_req, const int *ctx_ptr, const int *field,
                                                                        const int *feat, const float *val, CatalogItemSlots sl,
                                                                        CatalogDev cd, int max_row_nnz, int lds_cap) {
  static_assert(FMT == SERVE_F32 || FMT == SERVE_F16, "a packed table of w alone");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = wave_uniform(blockIdx.x * kPredRows + wv);
  if (r >= cd.rows) return;
  int4 *const E = wave_lds(smem, wv, lds_cap, 0).E;
  int nv = 0;
  catalog_stage_context(m, r, n_req, ctx_ptr, field, feat, val, max_row_nnz, lds_cap, lane, E, nv);
  const int lp = cd.lp / sl.n;  // of one slot's block
  catalog_u_store<FMT>(
      [&](int j) {
        const int a = j / lp;
        // (the slot's field and value by a chain of selects: sl lives in scalar registers, not in memory)
        int g = sl.field[0];
        float v = sl.val[0];
#pragma unroll
        for (int s = 1; s < kItemSlots; s++) {
          g = a == s ? sl.field[s] : g;
          v = a == s ? sl.val[s] : v;
        }
        return __fmul_rn(v, catalog_u_element<FMT>(m, E, nv, g, j - a * lp));
      },
      cd.lp, cd, r, lane);
}

// S_c of every item.  Four consecutive lanes share an item: lane q of them takes the vectors q, q + 4, ... of four
// factors of each of the m (m - 1) / 2 pairs' two slots (k % 4 == 0; else single factors q, q + 4, ...), and lane 0 the
// linear terms; two shuffles add the four partial sums.  A slot with an id outside [0, n_feats) is erased: its linear
// term and every pair it is in are skipped.  No LDS, no barrier.
// id[a]: slot a's id, or -1 for an erased slot and for every slot from sl.n on; q: the lane's place among its item's four.
// Returns S_c in all four lanes.  (catalog_dict_self_kernel, kernels_catalog_dict.h, resolves its ids otherwise and adds
// them by this function too.)
template <int FMT>
__device__ __forceinline__ float catalog_items_self_sum(const ModelDev &m, const CatalogItemSlots &sl, const int (&id)[kItemSlots], int q) {
  using Raw = typename WaveTable<FMT>::Raw;
  const int k = m.n_factors, L = m.row_len;
  float sum = 0.0f;
  if (q == 0) {
#pragma unroll
    for (int a = 0; a < kItemSlots; a++)
      if (id[a] >= 0) sum = __fmaf_rn(sl.val[a], m.lin_w[id[a]], sum);
  }
  const WaveTable<FMT> table(m);
#pragma unroll
  for (int a = 0; a < kItemSlots - 1; a++)
#pragma unroll
    for (int b = a + 1; b < kItemSlots; b++) {
      if (b >= sl.n || id[a] < 0 || id[b] < 0) continue;
      float dot = 0.0f;
      if ((k & 3) == 0) {
        const Raw *const x = table.slot(id[a], sl.field[b]), *const y = table.slot(id[b], sl.field[a]);
        for (int vi = q; vi < (k >> 2); vi += 4) {
          const float4 xf = serve_widen(x[vi]), yf = serve_widen(y[vi]);
          dot = __fmaf_rn(xf.x, yf.x, dot);
          dot = __fmaf_rn(xf.y, yf.y, dot);
          dot = __fmaf_rn(xf.z, yf.z, dot);
          dot = __fmaf_rn(xf.w, yf.w, dot);
        }
      } else {
        const int64_t xa = static_cast<int64_t>(id[a]) * L + sl.field[b] * k, ya = static_cast<int64_t>(id[b]) * L + sl.field[a] * k;
        for (int t = q; t < k; t += 4) {
          const float xf = FMT == SERVE_F16 ? serve_dec16(reinterpret_cast<const unsigned short *>(m.lat)[xa + t]) : m.lat[xa + t];
          const float yf = FMT == SERVE_F16 ? serve_dec16(reinterpret_cast<const unsigned short *>(m.lat)[ya + t]) : m.lat[ya + t];
          dot = __fmaf_rn(xf, yf, dot);
        }
      }
      sum = __fmaf_rn(__fmul_rn(sl.val[a], sl.val[b]), dot, sum);
    }
  sum = __fadd_rn(sum, __shfl_xor(sum, 1, 64));
  return __fadd_rn(sum, __shfl_xor(sum, 2, 64));
}

template <int FMT>
__global__ __launch_bounds__(256) void catalog_items_self_kernel(ModelDev m, CatalogItemSlots sl, const int *item_feat, int64_t n_items,
                                                                 float *item_s) {
  static_assert(FMT == SERVE_F32 || FMT == SERVE_F16, "a packed table of w alone");
  const int64_t c = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 2;
  const int q = threadIdx.x & 3;
  const bool live = c < n_items;  // (the four lanes of an item agree; idle lanes still take part in the shuffles)
  int id[kItemSlots];
#pragma unroll
  for (int a = 0; a < kItemSlots; a++) {
    id[a] = -1;
    if (live && a < sl.n) {
      const int i = item_feat[c * sl.n + a];
      id[a] = i >= 0 && i < m.n_feats ? i : -1;
    }
  }
  const float sum = catalog_items_self_sum<FMT>(m, sl, id, q);
  if (live && q == 0) item_s[c] = sum;
}

// The epilogue of one accumulator: the item's S_c, the request's base and (f16) shift.
template <int FMT>
__device__ __forceinline__ float catalog_items_logit(float a, float s, float base, int shift) {
  if (FMT == SERVE_F16) a = ldexpf(a, -shift);
  return __fadd_rn(a, __fadd_rn(s, base));
}

// The item source of catalog_accumulate and the two kernels (kernels_catalog.h "ROW SOURCES").  The kernels' common
// arguments then mean: tab row 0 of the whole table, lin the items' S_c, n_cand the items, v unused.
struct CatalogItemSrc {
  struct Args {
    const int *item_feat;  // [n_items][n_slots]
    int n_feats, n_slots;
    int chunks_per_row;    // Lp * ES / 256: chunks of one slot's block
  };
  using Term = CatalogNoTerm;
  static constexpr int kLdsInts = kItemSlots * 32;  // the ids of the wave's 32 items, [n_slots][32]; n_feats: reads as zeros
  const int *ids;
  int n_feats, chunks_per_row;
  int slot, first;  // of the chunk sought: its slot and that slot's chunk 0
  // (the wave's reads of the ids it parked for its last columns are behind catalog_accumulate's closing fence)
  __device__ __forceinline__ CatalogItemSrc(const Args &t, int *lds, int64_t c0, int64_t n_items, int lane)
      : ids(lds), n_feats(t.n_feats), chunks_per_row(t.chunks_per_row), slot(0), first(0) {
    for (int e = lane; e < 32 * t.n_slots; e += 64) {
      const int row = e / t.n_slots, a = e - row * t.n_slots;
      const int64_t c = c0 + row;
      int id = t.n_feats;  // (an erased slot and an item beyond the table: a row beyond the table's last)
      if (c < n_items) {
        id = t.item_feat[c * t.n_slots + a];
        if (id < 0 || id > t.n_feats) id = t.n_feats;
      }
      lds[a * 32 + row] = id;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  }
  __device__ __forceinline__ void seek(int ch) {
    if (ch == 0) slot = 0, first = 0;
    else if (ch - first == chunks_per_row) slot++, first = ch;
  }
  __device__ __forceinline__ uint4 load(const char *tab, int64_t row_bytes, int64_t, int row4, int it, int64_t, int ch, int sub,
                                        bool even16) const {
    return catalog_load(tab, row_bytes, ids[slot * 32 + row4 + 4 * it], n_feats, (ch - first) * kCatChunkBytes + 16 * sub, even16);
  }
  template <int FMT>
  static __device__ __forceinline__ float logit(float a, float, float s, float base, int shift) {
    return catalog_items_logit<FMT>(a, s, base, shift);
  }
};

}  // namespace ftrl_dev
