// kernels_catalog_lists.h -- request contexts against PER-REQUEST LISTS of items of a table (include/ffm_engine.h
// "Scoring a catalogue: per-request item lists"): the ranking call.  The table is kernels_catalog_items.h's (m <= 8
// slots in distinct fields, one value per slot), the score its formula,
//   score(r, c) = base_r + S_c + sum_a sum_{j < L} U_r^a[j] * W[c_a][j]              L = n_fields * n_factors
// but request r is scored against the items list_item[list_ptr[r] .. list_ptr[r + 1]) alone.
//
//   catalog_lists_u_kernel<FMT>      one wave per 128 elements of a request's m blocks U_r^a, v_a folded in: PLAIN FLOATS
//   catalog_lists_self_kernel<FMT>   four lanes per list entry: S of the listed items only (catalog_items_self_sum)
//   catalog_lists_kernel<FMT>        a workgroup per (request, 128 list positions): gathered fp32 dot products
//
// WHY NO MFMA  A request brings ONE row of the A operand (its U) and a list of its own: nothing of the B operand
// (the gathered table rows) is shared between two requests, so a 32x32 tile would carry 1 useful row in 32 -- and
// padding the tile with other requests' U rows would multiply every list by every other request's context, which is
// score_items on the union of the lists.  What is left is a batch of matrix-vector products whose matrix is read once:
// a gather-bound kernel, 2 flops per element loaded, on the VALU.
//
// OPERANDS AND WORK SPLIT (catalog_lists_kernel)
//   U  float [n_req][m][Lu], Lu = L rounded up to 8 floats and zero-filled, the elements catalog_u_element<FMT>'s times
//     v_a: on f16 too plain fp32 -- no hi / lo planes, no shift; the VALU multiplies fp32.  Per slot a the workgroup
//     copies U_r^a into one of two LDS buffers of Lu floats (dynamic LDS, 2 * 4 * Lu bytes: 5 KB at 39 x 16) and meets
//     at ONE barrier: slot a + 1 is written into the other buffer while late waves still read a, and a is written again
//     only behind the barrier of a + 1, which every wave reaches with its reads of a done.
//   W  A group of 16 lanes (one DPP row) owns 8 list positions of the workgroup's 128, four at a time: group g takes
//     positions 64 t + 4 g + i, t < 2, i < 4.  Lane s of the group loads the 16-byte vectors s, s + 16, ... of each of
//     the four rows W[c_a] -- 256 consecutive bytes of a row per step and row, four rows' loads in flight together,
//     the step loop unrolled twice -- decodes them by the table's own decode (serve_dec16x4 on f16) and multiplies them
//     with the same vectors of U from LDS: the four groups of a wave read the same LDS addresses (a broadcast).  Rows
//     that are only 8-byte aligned (f16, L % 8 != 0: 3 fields x 4 factors) come as two halves (catalog_load), the
//     missing half of the last vector as zeros against U's zero fill.  An erased slot (id outside [0, n_feats)) and
//     every slot of a list entry outside [0, n_items) load NOTHING: zero registers.
//   ids  item_feat[c][a] of the group's eight positions is read per slot, right behind the barrier; the eight items
//     themselves once, before the slot loop.
//   sums  One fp32 accumulator per position and lane, carried across the slots: fma in the order (slot, vector, element).
//     The 16 partial sums of a position are added by xor shuffles 8, 4, 2, 1.  Which lane holds which elements, and the
//     order of every addition, is a function of (slot, element) alone: a score's bits depend on (request, item) and not
//     on the position in the list, the list's length or what else is in the call.
//   epilogue  fadd(acc, fadd(S, base_r)) -- catalog_items_logit<SERVE_F32> -- then sigmoid_ref under output_prob.  Lanes
//     0 .. 3 of a group store its positions 4 g .. 4 g + 3: 16 consecutive floats per wave.  out is indexed in 64 bits.
//   bounds  A workgroup whose segment starts beyond its list leaves before the first barrier (the whole workgroup
//     agrees).  A list is read up to min(its length, list_cap, n_list - list_ptr[r]); a list_ptr pair that is negative
//     or descends scores nothing.  No load or store of a position beyond that.
// SEG = 128 AND NOT 64 OR 256: 64 positions (one batch per group) restage U once per 64 rows gathered, 256 double the
// accumulators, ids and items a lane carries (48 more VGPRs) for the same loads in flight; at 128 the headline lists of
// 512 are four workgroups per request.
//
// NOT BIT FOR BIT against rows or score_items; for finite tables, N = m L + m + m (m - 1) / 2 k,
//   |score - (base_r + ref64)| <= (N + 32) * 2^-24 * (|base_r| + scale)          (score_items_reference, engine.py)
// -- the any-order bound of fp32 sums, which a chain of fp32 FMAs and a tree of fp32 adds satisfy.
//
// RESOURCES (hipcc --offload-arch=gfx950 -O3, kernel-resource-usage; no scratch in any of them)
//   catalog_lists_u_kernel<f32>      16 VGPRs, 8 waves per SIMD      <f16>   16 VGPRs, 8 waves
//   catalog_lists_self_kernel<f32>   38 VGPRs, 8 waves               <f16>   32 VGPRs, 8 waves   (catalog_items_self_kernel's counts)
//   catalog_lists_kernel<f32>        96 VGPRs, 5 waves               <f16>  100 VGPRs, 4 waves   (no static LDS; dynamic as above)
// The hot kernel's registers are the two unrolled steps' eight 16-byte vectors in flight (32), eight accumulators, ids and
// items, and the addresses of four rows.
#pragma once
#include "kernels_catalog_items.h"

namespace ftrl_dev {

constexpr int kListLanes = 16;                                // lanes of a group: one DPP row
constexpr int kListAhead = 4;                                 // positions of a group with their loads in flight together
constexpr int kListPass = 256 / kListLanes * kListAhead;      // positions a workgroup takes per pass: 64
constexpr int kListSeg = 2 * kListPass;                       // positions a workgroup owns: 128
constexpr int kListOwn = kListSeg / (256 / kListLanes);       // positions a group owns: 8
constexpr int kListURun = 128;                                // elements of U a wave of catalog_lists_u_kernel writes: two per lane
constexpr int kListMaxLu = 8192;                              // floats of a U block both LDS buffers hold in 64 KB

// L in whole vectors of eight elements (16 bytes of an f16 row): the length of one slot's block of U
__host__ __device__ inline int catalog_lists_lu(int L) { return (L + 7) / 8 * 8; }

// One wave per (request, run of kListURun consecutive elements of its m * lu); kPredRows waves per workgroup, `parts`
// runs per request.  u: float [n_req][sl.n][lu].  (One wave per REQUEST, as catalog_items_u_kernel has it, is 82 us at 38
// context entries and 3 slots whatever the lists are -- every element scans the staged context, 30 elements per lane one
// after another -- and was twice the time of the dot products; a run per wave stages the context once per run instead,
// which is a few dozen entries.)
template <int FMT>
__global__ __launch_bounds__(64 * kPredRows) void catalog_lists_u_kernel(ModelDev m, int n_req, const int *ctx_ptr, const int *field,
                                                                        const int *feat, const float *val, CatalogItemSlots sl, float *u,
                                                                        int lu, int parts, int max_row_nnz, int lds_cap) {
  static_assert(FMT == SERVE_F32 || FMT == SERVE_F16, "a packed table of w alone");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int w = wave_uniform(blockIdx.x * kPredRows + wv);
  const int r = w / parts, part = w - r * parts;
  if (r >= n_req) return;
  int4 *const E = wave_lds(smem, wv, lds_cap, 0).E;
  int nv = 0;
  catalog_stage_context(m, r, n_req, ctx_ptr, field, feat, val, max_row_nnz, lds_cap, lane, E, nv);
  float *const U = u + static_cast<int64_t>(r) * sl.n * lu;
  const int end = min((part + 1) * kListURun, sl.n * lu);
  for (int j = part * kListURun + lane; j < end; j += 64) {
    const int a = j / lu;
    int g = sl.field[0];
    float v = sl.val[0];
#pragma unroll
    for (int s = 1; s < kItemSlots; s++) {
      g = a == s ? sl.field[s] : g;
      v = a == s ? sl.val[s] : v;
    }
    U[j] = __fmul_rn(v, catalog_u_element<FMT>(m, E, nv, g, j - a * lu));
  }
}

// S of list entry p = S_c of item list_item[p], by the function that gives score_items its S_c: the same bits.  An
// entry outside [0, n_items) is an item whose slots are all erased: 0.
template <int FMT>
__global__ __launch_bounds__(256) void catalog_lists_self_kernel(ModelDev m, CatalogItemSlots sl, const int *item_feat, int n_items,
                                                                 const int *list_item, int64_t n_list, float *list_s) {
  static_assert(FMT == SERVE_F32 || FMT == SERVE_F16, "a packed table of w alone");
  const int64_t p = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 2;
  const int q = threadIdx.x & 3;
  const bool live = p < n_list;  // (the four lanes of an entry agree; idle lanes still take part in the shuffles)
  const int c = live ? list_item[p] : -1;
  const bool inside = c >= 0 && c < n_items;
  int id[kItemSlots];
#pragma unroll
  for (int a = 0; a < kItemSlots; a++) {
    id[a] = -1;
    if (inside && a < sl.n) {
      const int i = item_feat[static_cast<int64_t>(c) * sl.n + a];
      id[a] = i >= 0 && i < m.n_feats ? i : -1;
    }
  }
  const float sum = catalog_items_self_sum<FMT>(m, sl, id, q);
  if (live && q == 0) list_s[p] = sum;
}

// acc += the dot product of the eight (f16) or four (f32) elements of table vector w with U's floats at u.
template <int FMT>
__device__ __forceinline__ float catalog_lists_fma(uint4 w, const float4 *u, float acc) {
  if constexpr (FMT == SERVE_F16) {
    const float4 x = serve_dec16x4(make_uint2(w.x, w.y)), y = serve_dec16x4(make_uint2(w.z, w.w));
    const float4 p = u[0], q = u[1];
    acc = __fmaf_rn(p.x, x.x, acc);
    acc = __fmaf_rn(p.y, x.y, acc);
    acc = __fmaf_rn(p.z, x.z, acc);
    acc = __fmaf_rn(p.w, x.w, acc);
    acc = __fmaf_rn(q.x, y.x, acc);
    acc = __fmaf_rn(q.y, y.y, acc);
    acc = __fmaf_rn(q.z, y.z, acc);
    acc = __fmaf_rn(q.w, y.w, acc);
  } else {
    const float4 p = u[0];
    acc = __fmaf_rn(p.x, __uint_as_float(w.x), acc);
    acc = __fmaf_rn(p.y, __uint_as_float(w.y), acc);
    acc = __fmaf_rn(p.z, __uint_as_float(w.z), acc);
    acc = __fmaf_rn(p.w, __uint_as_float(w.w), acc);
  }
  return acc;
}

// Grid (n_req, cdiv(list_cap, kListSeg)): request blockIdx.x, list positions [kListSeg * blockIdx.y, ...).  tab: row 0
// of the table; u, lu: catalog_lists_u_kernel's; list_s: catalog_lists_self_kernel's; base [n_req]: the row kernel's.
template <int FMT>
__global__ __launch_bounds__(256) void catalog_lists_kernel(const char *tab, int L, int n_feats, int m, const int *item_feat, int n_items,
                                                            const int *list_ptr, const int *list_item, int64_t n_list, int list_cap,
                                                            const float *u, int lu, const float *list_s, const float *base,
                                                            int output_prob, float *out) {
  static_assert(FMT == SERVE_F32 || FMT == SERVE_F16, "a packed table of w alone");
  constexpr int ES = FMT == SERVE_F16 ? 2 : 4, VF = 16 / ES / 4;  // float4s of U per table vector
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4 *const ub = reinterpret_cast<float4 *>(smem);  // two buffers of lu floats
  const int r = blockIdx.x;
  const int64_t b = list_ptr[r], e = list_ptr[r + 1];
  if (b < 0 || e < b) return;
  const int len = static_cast<int>(min(min(e, n_list) - b, static_cast<int64_t>(list_cap)));
  const int seg0 = blockIdx.y * kListSeg;
  if (seg0 >= len) return;  // (the whole workgroup: nobody waits at a barrier below)
  const int g = threadIdx.x / kListLanes, s = threadIdx.x % kListLanes;
  const int64_t row_bytes = static_cast<int64_t>(L) * ES;
  const bool even16 = (row_bytes & 15) == 0;
  const int n_vec = static_cast<int>((row_bytes + 15) >> 4);

  // the group's positions: x = 4 t + i is position seg0 + kListPass t + 4 g + i; its item, -1 for none
  int item[kListOwn];
  float acc[kListOwn];
#pragma unroll
  for (int x = 0; x < kListOwn; x++) {
    const int pos = seg0 + kListPass * (x / kListAhead) + kListAhead * g + x % kListAhead;
    int c = -1;
    if (pos < len) c = list_item[b + pos];
    item[x] = c >= 0 && c < n_items ? c : -1;
    acc[x] = 0.0f;
  }

  for (int a = 0; a < m; a++) {
    float4 *const ua = ub + (a & 1) * (lu / 4);
    const float4 *const src = reinterpret_cast<const float4 *>(u + (static_cast<int64_t>(r) * m + a) * lu);
    for (int j = threadIdx.x; j < lu / 4; j += 256) ua[j] = src[j];
    int id[kListOwn];  // n_feats: an erased slot, which catalog_load reads as zero registers
#pragma unroll
    for (int x = 0; x < kListOwn; x++) {
      int i = n_feats;
      if (item[x] >= 0) i = item_feat[static_cast<int64_t>(item[x]) * m + a];
      id[x] = i >= 0 && i < n_feats ? i : n_feats;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kListOwn / kListAhead; t++) {
      if (seg0 + kListPass * t + kListAhead * g >= len) continue;  // (none of the four: the group agrees)
#pragma unroll 2
      for (int v = s; v < n_vec; v += kListLanes) {
        uint4 w[kListAhead];
#pragma unroll
        for (int i = 0; i < kListAhead; i++) w[i] = catalog_load(tab, row_bytes, id[kListAhead * t + i], n_feats, 16 * v, even16);
#pragma unroll
        for (int i = 0; i < kListAhead; i++) acc[kListAhead * t + i] = catalog_lists_fma<FMT>(w[i], ua + VF * v, acc[kListAhead * t + i]);
      }
    }
  }

  // ---- the 16 partial sums of each position, in one fixed order; then lane i < 4 of the group has position 4 g + i
  const float base_r = base[r];
#pragma unroll
  for (int t = 0; t < kListOwn / kListAhead; t++) {
    float mine = 0.0f;
#pragma unroll
    for (int i = 0; i < kListAhead; i++) {
      float x = acc[kListAhead * t + i];
#pragma unroll
      for (int d = kListLanes / 2; d >= 1; d >>= 1) x = __fadd_rn(x, __shfl_xor(x, d, 64));
      mine = s == i ? x : mine;
    }
    const int pos = seg0 + kListPass * t + kListAhead * g + s;
    if (s < kListAhead && pos < len) {
      const float score = catalog_items_logit<SERVE_F32>(mine, list_s[b + pos], base_r, 0);
      out[b + pos] = output_prob ? sigmoid_ref(score) : score;
    }
  }
}

}  // namespace ftrl_dev
