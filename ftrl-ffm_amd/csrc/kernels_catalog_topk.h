// kernels_catalog_topk.h -- the best K candidates per request of a catalogue (include/ffm_engine.h "Scoring a
// catalogue: the best K"): kernels_catalog.h's contraction with a selection in place of the store.  The matrix of
// scores is never written.
//
//   catalog_topk_kernel<FMT, RT>   a bounded grid; workgroup b takes the 128-candidate slabs b, b + gridDim.x, ...,
//                                  each of its four waves its 32 candidates of every slab, against RT request tiles
//   catalog_topk_merge_kernel      one workgroup per request: its gridDim.x * 4 partial lists into the K slots
//
// ORDER  a candidate's key is one 64-bit word, the larger first:
//   key = key32(logit) << 32 | ~uint32(column)      key32: all bits of a negative float flipped, the sign bit of any other
// so -0.0 < +0.0, a NaN with a clear sign bit lies above +inf, and equal logits go to the lower id.  Keys are unique
// and never 0 (column < 2^31: ~column has its top bit set), so 0 stands for an empty slot and nothing rests on the
// order in which partial results meet.  The logit is catalog_accumulate's accumulator through catalog_logit: the bits
// catalog_gemm_kernel stores for the same request and candidate, whatever RT either launch runs with.
//
// SELECTION (per wave, no workgroup barrier)  In dynamic LDS every wave keeps one list of Kp = top_k rounded up to a
// power of two keys per request of its 32 RT, slot s of request i of tile t at word (t Kp + s) * 32 + i: lanes on
// consecutive words.  After a slab's accumulation the wave writes a tile's 32 x 32 logits request-major into its own
// operand tile (free by then; rows of 36 floats, 4.5 of its 8.5 KB), behind a wave fence.  Lane i < 32 owns request i:
// it reads its 32 logits as float4 and compares their keys with its list's minimum, which it holds in registers; a
// wave-wide ballot of "some key beats my minimum" skips the rest, the common case after the first few slabs (about
// K (1 + ln(span / K)) insertions per request over a span of candidates).  An insertion overwrites the minimum and
// rescans the list's top_k slots for the new one.  Candidates from n_cand on and requests from n_req on are guarded
// out of the scan: their keys never enter a list.  At the end the wave copies its lists to
// part[request][blockIdx.x * 4 + wave][Kp], 64-bit words under 64-bit indices, lanes along the list.  A wave without
// candidates stores its empty lists like any other: nothing returns early.
//
// MERGE  256 threads stream the request's P * Kp words, 16 bytes a thread and four such loads in flight, past the
// value of the top_k-th best key so far (0 at first: empty slots drop out by themselves); survivors are appended to
// a tile of 1024 keys in LDS behind the best so far, and when fewer than 512 slots are left, and at the end, the tile
// is sorted descending by a bitonic network.  Slot j < top_k then gets id cand_first + ~low word and the float
// recovered from key32 (its sigmoid under output_prob); an empty slot, and every slot of a request whose base is NaN
// (a flagged context), gets id -1 and the NaN 0x7FC00000.
//
// LDS per workgroup of catalog_topk_kernel: 34 816 bytes of operand tiles + 1024 RT Kp bytes of lists + 1024 RT
// bytes of the requests' base and shift (staged once: read from registers they cost 16 RT VGPRs each)
//   K <= 8: RT 4, 32 + 4 KB     K <= 16: RT 2, 32 + 2 KB     K <= 32: RT 1, 32 + 1 KB     K <= 64: RT 1, 64 + 1 KB
// (engine_select.h: catalog_topk_rt).  Plain vector stores only.
//
// RESOURCES (hipcc --offload-arch=gfx950 -O3, kernel-resource-usage; no scratch in any of them)
//   catalog_topk_kernel<f32, 1>    97 VGPRs, 16 AGPRs      <f16, 1>   91 VGPRs, 16 AGPRs
//   catalog_topk_kernel<f32, 2>   102 VGPRs, 32 AGPRs      <f16, 2>  104 VGPRs, 32 AGPRs
//   catalog_topk_kernel<f32, 4>   129 VGPRs, 64 AGPRs      <f16, 4>  135 VGPRs, 64 AGPRs
//   catalog_topk_merge_kernel      31 VGPRs, 8 200 bytes of LDS
//   Registers admit 4, 3 and 2 waves per SIMD at RT 1, 2 and 4; LDS admits fewer (two workgroups per CU up to K = 32,
//   one at K = 64) and is what binds (profiles/score_catalog_topk.md).
//   (catalog_gemm_kernel's own counts, kernels_catalog.h, are what they were before catalog_accumulate was factored out)
#pragma once
#include "kernels_catalog.h"

namespace ftrl_dev {

constexpr int kTopkMax = 64;          // top_k at the most
constexpr int kTopkRowFloats = 36;    // a request's 32 logits in the wave's tile: 144-byte rows, float4 reads on all banks
constexpr int kTopkMergeThreads = 256;
constexpr int kTopkTile = 1024;       // keys the merge sorts at a time
constexpr unsigned kTopkNaN = 0x7FC00000u;
static_assert(32 * kTopkRowFloats * 4 <= 32 * kCatRowBytes, "the logits fit the wave's operand tile");

__host__ __device__ inline int catalog_topk_kp(int top_k) {
  int kp = 1;
  while (kp < top_k) kp <<= 1;
  return kp;
}
__host__ __device__ inline size_t catalog_topk_lds_bytes(int rt, int kp) {
  return static_cast<size_t>(kCatWaves) * kCatTile * rt * (kp * sizeof(unsigned long long) + sizeof(float) + sizeof(int));
}

__device__ __forceinline__ unsigned topk_key32(float x) {
  const unsigned b = __float_as_uint(x);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float topk_unkey32(unsigned k) { return __uint_as_float((k >> 31) ? k ^ 0x80000000u : ~k); }

// Requests [r0, r0 + 32 RT) against all n_cand candidates of the range (over another row source: its n_cand columns,
// as catalog_gemm_kernel); kp: catalog_topk_kp(top_k); part[n_req][gridDim.x * 4][kp].  Dynamic LDS:
// catalog_topk_lds_bytes(RT, kp).
template <int FMT, int RT, typename Src = CatalogSlabSrc>
__global__ __launch_bounds__(64 * kCatWaves) void catalog_topk_kernel(const char *tab, const float *lin, int L, CatalogDev cd, int r0,
                                                                     int n_req, int64_t n_cand, float v, int top_k, int kp,
                                                                     unsigned long long *part, typename Src::Args args) {
  static_assert(FMT == SERVE_F32 || FMT == SERVE_F16, "a packed table of w alone");
  static_assert(RT == 1 || RT == 2 || RT == 4, "request tiles per launch");
  __shared__ __attribute__((aligned(16))) char tile[kCatWaves][32 * kCatRowBytes];
  __shared__ int own[kCatWaves][Src::kLdsInts > 0 ? Src::kLdsInts : 1];  // (as catalog_gemm_kernel's)
  extern __shared__ __attribute__((aligned(16))) unsigned long long topk_lists[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  char *const T = tile[wv];
  float *const S = reinterpret_cast<float *>(T);  // the logits of one tile: [32 requests][kTopkRowFloats]
  unsigned long long *const Lw = topk_lists + static_cast<size_t>(wv) * kCatTile * RT * kp;
  // behind all lists: base and shift of the wave's requests (read 16 RT times a slab: from here, not from registers)
  float *const Bw = reinterpret_cast<float *>(topk_lists + static_cast<size_t>(kCatWaves) * kCatTile * RT * kp) + wv * 2 * kCatTile * RT;
  int *const Hw = reinterpret_cast<int *>(Bw + kCatTile * RT);
  for (int e = lane; e < kCatTile * RT * kp; e += 64) Lw[e] = 0ull;
  for (int e = lane; e < kCatTile * RT; e += 64) {
    const bool live = r0 + e < n_req;
    Bw[e] = live ? cd.base[r0 + e] : 0.0f;
    Hw[e] = live && FMT == SERVE_F16 ? cd.shift[r0 + e] : 0;
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");

  unsigned long long mn[RT];  // the smallest key of the list of request j of tile t, and its slot (lanes < 32)
  int mn_at[RT];
#pragma unroll
  for (int t = 0; t < RT; t++) mn[t] = 0ull, mn_at[t] = 0;

  const int64_t n_slabs = (n_cand + kCatCands - 1) / kCatCands;
  for (int64_t slab = blockIdx.x; slab < n_slabs; slab += gridDim.x) {
    const int64_t c0 = slab * kCatCands + wv * 32;  // the wave's first candidate of the slab
    if (c0 >= n_cand) break;                        // (its later slabs lie beyond too; the final store still runs)
    cat_v16f acc[RT];
    catalog_accumulate<FMT, RT>(tab, L, cd, r0, c0, n_cand, T, lane, acc, Src(args, own[wv], c0, n_cand, lane));
    const int64_t c = c0 + j;
    const float lw = c < n_cand ? lin[c] : 0.0f;
    const int n_col = static_cast<int>(n_cand - c0 < 32 ? n_cand - c0 : 32);  // columns of the tile that are candidates
    const typename Src::Term term(args, c, n_cand);
#pragma unroll
    for (int t = 0; t < RT; t++) {
      term.template add<FMT>(acc[t], r0 + kCatTile * t, h, Hw + kCatTile * t);
#pragma unroll
      for (int x = 0; x < 16; x++) {
        const int row = 8 * (x >> 2) + 4 * h + (x & 3), q = kCatTile * t + row;
        if (r0 + q < n_req) S[row * kTopkRowFloats + j] = Src::template logit<FMT>(acc[t][x], v, lw, Bw[q], FMT == SERVE_F16 ? Hw[q] : 0);
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      const bool mine = h == 0 && r0 + kCatTile * t + j < n_req;
      const float4 *const row4 = reinterpret_cast<const float4 *>(S + j * kTopkRowFloats);
      const unsigned low0 = ~static_cast<unsigned>(c0);  // ~(c0 + col) == low0 - col
      bool beats = false;
      if (mine) {
        const unsigned mn_hi = static_cast<unsigned>(mn[t] >> 32);  // (a tie in key32 may still beat it: decided below)
#pragma unroll
        for (int q = 0; q < 8; q++) {
          const float4 s = row4[q];
          beats = beats || (4 * q + 0 < n_col && topk_key32(s.x) >= mn_hi) || (4 * q + 1 < n_col && topk_key32(s.y) >= mn_hi) ||
                  (4 * q + 2 < n_col && topk_key32(s.z) >= mn_hi) || (4 * q + 3 < n_col && topk_key32(s.w) >= mn_hi);
        }
      }
      if (__ballot(beats) != 0ull) {
        if (beats) {
          unsigned long long *const lst = Lw + static_cast<size_t>(t) * kp * 32 + j;  // slot s at lst[32 s]
#pragma unroll 1
          for (int col = 0; col < n_col; col++) {
            const unsigned long long key =
                static_cast<unsigned long long>(topk_key32(S[j * kTopkRowFloats + col])) << 32 | (low0 - static_cast<unsigned>(col));
            if (key <= mn[t]) continue;
            lst[32 * mn_at[t]] = key;
            unsigned long long m = lst[0];
            int at = 0;
#pragma unroll 1
            for (int s = 1; s < top_k; s++) {
              const unsigned long long k2 = lst[32 * s];
              if (k2 < m) m = k2, at = s;
            }
            mn[t] = m;
            mn_at[t] = at;
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // (the tile is written again: the next t, the next slab)
    }
  }

  // ---- the wave's lists: part[r][blockIdx.x * 4 + wv][kp], lanes along the list
  const int64_t P = static_cast<int64_t>(gridDim.x) * kCatWaves, p = static_cast<int64_t>(blockIdx.x) * kCatWaves + wv;
  const int kp_log = __ffs(kp) - 1;
  for (int e = lane; e < kCatTile * RT * kp; e += 64) {
    const int q = e >> kp_log, s = e & (kp - 1);  // request q of the wave's 32 RT, slot s
    const int r = r0 + q;
    if (r < n_req) part[(static_cast<int64_t>(r) * P + p) * kp + s] = Lw[(static_cast<size_t>(q >> 5) * kp + s) * 32 + (q & 31)];
  }
}

// The tile's 1024 keys into descending order; every thread of the workgroup, barriers inside.
__device__ __forceinline__ void topk_sort_tile(unsigned long long *buf) {
  for (int k = 2; k <= kTopkTile; k <<= 1)
    for (int d = k >> 1; d > 0; d >>= 1) {
      for (int pr = threadIdx.x; pr < kTopkTile / 2; pr += kTopkMergeThreads) {
        const int i = ((pr & ~(d - 1)) << 1) | (pr & (d - 1)), l = i + d;
        const unsigned long long a = buf[i], b = buf[l];
        if ((a < b) == ((i & k) == 0)) buf[i] = b, buf[l] = a;
      }
      __syncthreads();
    }
}

// Workgroup r: request r's P lists of kp words (P a multiple of four; 0: no candidates) into out_score / out_id [r][top_k].
// base: the requests' own logits (a NaN marks a flagged context), or null.
__global__ __launch_bounds__(kTopkMergeThreads) void catalog_topk_merge_kernel(const unsigned long long *part, int64_t P, int kp, int top_k,
                                                                              const float *base, int cand_first, int output_prob,
                                                                              float *out_score, int *out_id) {
  __shared__ __attribute__((aligned(16))) unsigned long long buf[kTopkTile];
  __shared__ int cnt;
  const int r = blockIdx.x, tid = threadIdx.x;
  for (int e = tid; e < kTopkTile; e += kTopkMergeThreads) buf[e] = 0ull;
  if (tid == 0) cnt = 0;
  __syncthreads();
  const int64_t total = P * kp;  // (a multiple of four words, and so is every list's start: 16-byte loads stay inside)
  const ulonglong2 *const src = reinterpret_cast<const ulonglong2 *>(part + static_cast<int64_t>(r) * total);
  const int64_t n_vec = total / 2;
  unsigned long long thr = 0ull;  // keys at or below it cannot reach the first top_k
  constexpr int kAhead = 4;       // loads of a thread in flight: 4 * 256 * 2 = 2048 keys a round
  for (int64_t v0 = 0; v0 < n_vec; v0 += kAhead * kTopkMergeThreads) {
    ulonglong2 in[kAhead];
#pragma unroll
    for (int a = 0; a < kAhead; a++) {
      const int64_t at = v0 + a * kTopkMergeThreads + tid;
      in[a] = at < n_vec ? src[at] : make_ulonglong2(0ull, 0ull);
    }
#pragma unroll
    for (int a = 0; a < kAhead; a++) {
      if (v0 + a * kTopkMergeThreads >= n_vec) break;  // (uniform)
      if (in[a].x > thr) buf[atomicAdd(&cnt, 1)] = in[a].x;  // at most 512 a step: the tile holds them (cnt <= 512 here)
      if (in[a].y > thr) buf[atomicAdd(&cnt, 1)] = in[a].y;
      __syncthreads();
      const int filled = cnt;
      __syncthreads();
      if (filled > kTopkTile / 2) {
        topk_sort_tile(buf);
        thr = buf[top_k - 1];
        __syncthreads();
        for (int e = top_k + tid; e < kTopkTile; e += kTopkMergeThreads) buf[e] = 0ull;
        if (tid == 0) cnt = top_k;
        __syncthreads();
      }
    }
  }
  topk_sort_tile(buf);
  const bool flagged = base != nullptr && base[r] != base[r];
  for (int s = tid; s < top_k; s += kTopkMergeThreads) {
    const unsigned long long key = buf[s];
    const int64_t at = static_cast<int64_t>(r) * top_k + s;
    if (key == 0ull || flagged) {
      out_id[at] = -1;
      out_score[at] = __uint_as_float(kTopkNaN);
    } else {
      const float logit = topk_unkey32(static_cast<unsigned>(key >> 32));
      out_id[at] = cand_first + static_cast<int>(~static_cast<unsigned>(key));
      out_score[at] = output_prob ? sigmoid_ref(logit) : logit;
    }
  }
}

}  // namespace ftrl_dev
