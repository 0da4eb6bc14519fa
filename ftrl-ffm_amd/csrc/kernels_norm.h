// kernels_norm.h -- FFM_FLAG_NORM_ROWS (include/ffm_engine.h "Normalised rows"): every row of a block scaled to
// unit Euclidean length, in HBM, behind the block's upload and id rewriting and ahead of every kernel that reads
// val.  Host side: engine_norm.h.
//
// The definition is sequential per row -- s = fl(s + fl(v * v)) over the kept entries in entry order, then
// scale = fl(1 / fl(sqrt(s))) -- so a lane sums one row; what a workgroup shares is the memory traffic.  It takes
// a RUN of kNormRows (64) consecutive rows, whose entries are one contiguous span of val / feat / field:
//   1  the span comes in with 16-byte loads, lane after lane; each entry leaves fl(v * v) in LDS, or +0 where the
//      model does not keep the entry (s + 0 == s for every s the sum can hold, NaN and inf included);
//   2  lane r sums row r out of LDS in entry order, works out the scale and writes it over the row's squares;
//   3  the span is read again (an L2 hit: this workgroup just loaded it) and goes out as fl(v * scale), 16 bytes per lane.
// The vector part covers the 16-byte groups that lie whole inside the span; the up to three entries in front and
// behind go singly, so no workgroup writes a group it shares with its neighbour, and arrays that are not
// 16-byte aligned (vec == 0) go singly altogether.  LDS index = entry - (span's start rounded down to 4): a
// group's four floats are one aligned LDS vector.  Lane r's reads in step 2 are a stride of its row length
// apart: conflict-free for odd lengths (39), 2^k-way for a multiple of 2^k -- 10 KB at LDS rate either way.
// The run is short on purpose: the kernel is bound by latency, not by bytes -- steps 1 and 3 are a few dependent
// trips to memory per lane and step 2 one wave's chain of LDS reads -- so what counts is how many workgroups
// share a block: 128 for 8192 rows.  (Runs of 256 rows, 32 workgroups: 59 us for the headline block; see
// profiles/row_norm.md.)  A run whose span does not fit kNormCap (rows beyond 64 entries on average) takes the
// plain path: lane r walks row r in global memory.  Rows left unscaled (s zero, infinite or NaN) are counted by ballot, one atomic per wave.
// Every operation is a rounding of its own: no FMA, IEEE sqrt and divide, denormals kept (norm_square .. norm_scale).
#pragma once

namespace ftrl_dev {

constexpr int kNormThreads = 256;
constexpr int kNormRows = 64;     // rows of a run: one per lane of the first wave
constexpr int kNormCap = 4096;    // entries of a run that LDS holds (16 KB)

// The block as the kernel takes it.  field == nullptr or n_fields == 0: the entry's id alone decides (LR / FM; FFM
// rows of one entry per field in field order).  val_in == nullptr: every value is 1.0f.  val_out may be val_in.
struct NormJob {
  int n_rows, nnz;
  const int *row_ptr, *field, *feat;
  const float *val_in;
  float *val_out;
  int n_feats, n_fields;
  int vec;  // feat, field, val_in and val_out are all 16-byte aligned
  unsigned long long *unscaled;
};

// stage_row's predicate (kernels_row.h) on the ids as the kernels see them.
__host__ __device__ inline bool norm_keeps(int feat, int field, int n_feats, int n_fields) {
  return static_cast<unsigned>(feat) < static_cast<unsigned>(n_feats) &&
         (n_fields <= 0 || static_cast<unsigned>(field) < static_cast<unsigned>(n_fields));
}
__host__ __device__ inline bool norm_scales(float s) { return s > 0.0f && s < __builtin_inff(); }

// The arithmetic, the project's habit (ftrl_math.h): plain operators under -ffp-contract=off and hipcc's default
// correctly rounded fp32 sqrt and divide -- and, so that no build flag can change it, contraction off right here.
__device__ __forceinline__ float norm_square(float v, bool keep) {
#pragma clang fp contract(off)
  return keep ? v * v : 0.0f;
}
__device__ __forceinline__ float norm_add(float s, float sq) {
#pragma clang fp contract(off)
  return s + sq;
}
// (a row that is not scaled keeps its bits, a signalling NaN's included)
__device__ __forceinline__ float norm_apply(float v, float scale) {
#pragma clang fp contract(off)
  return scale == 1.0f ? v : v * scale;
}
__device__ __forceinline__ float norm_scale(float s) {
#pragma clang fp contract(off)
  return norm_scales(s) ? 1.0f / sqrtf(s) : 1.0f;
}
__device__ __forceinline__ int norm_clamp(int x, int lo, int hi) { return x < lo ? lo : x > hi ? hi : x; }

__global__ __launch_bounds__(kNormThreads) void normalize_rows_kernel(NormJob j) {
  __shared__ __attribute__((aligned(16))) float lds[kNormCap];
  const int tid = threadIdx.x;
  const int n_runs = (j.n_rows + kNormRows - 1) / kNormRows;
  const bool fielded = j.field != nullptr && j.n_fields > 0;
  const int F = fielded ? j.n_fields : 0;
  for (int run = blockIdx.x; run < n_runs; run += gridDim.x) {
    const int r0 = run * kNormRows, nr = min(kNormRows, j.n_rows - r0);
    // (row_ptr is the caller's on the _device call: nothing below leaves [0, nnz) whatever it holds)
    const int base = norm_clamp(j.row_ptr[r0], 0, j.nnz), end = norm_clamp(j.row_ptr[r0 + nr], base, j.nnz);
    const int off = base & ~3;
    int b = base, e = base;
    if (tid < nr) {
      b = norm_clamp(j.row_ptr[r0 + tid], base, end);
      e = norm_clamp(j.row_ptr[r0 + tid + 1], b, end);
    }
    bool unscaled = false;
    if (end - off <= kNormCap) {  // (the same in every lane of the workgroup)
      // the 16-byte groups whole inside the span: [a_lo, a_hi); in front and behind: n_head + n_tail single entries
      const int a_lo = j.vec ? min((base + 3) & ~3, end) : base;
      const int a_hi = j.vec ? max(a_lo, end & ~3) : base;
      const int n_head = a_lo - base, n_edge = n_head + (end - a_hi);
      for (int q = (a_lo >> 2) + tid; q < (a_hi >> 2); q += kNormThreads) {
        const float4 v = j.val_in ? reinterpret_cast<const float4 *>(j.val_in)[q] : make_float4(1.0f, 1.0f, 1.0f, 1.0f);
        const int4 ft = reinterpret_cast<const int4 *>(j.feat)[q];
        const int4 fl = fielded ? reinterpret_cast<const int4 *>(j.field)[q] : make_int4(0, 0, 0, 0);
        float4 sq;
        sq.x = norm_square(v.x, norm_keeps(ft.x, fl.x, j.n_feats, F));
        sq.y = norm_square(v.y, norm_keeps(ft.y, fl.y, j.n_feats, F));
        sq.z = norm_square(v.z, norm_keeps(ft.z, fl.z, j.n_feats, F));
        sq.w = norm_square(v.w, norm_keeps(ft.w, fl.w, j.n_feats, F));
        *reinterpret_cast<float4 *>(&lds[(q << 2) - off]) = sq;
      }
      for (int i = tid; i < n_edge; i += kNormThreads) {
        const int p = i < n_head ? base + i : a_hi + (i - n_head);
        const float v = j.val_in ? j.val_in[p] : 1.0f;
        lds[p - off] = norm_square(v, norm_keeps(j.feat[p], fielded ? j.field[p] : 0, j.n_feats, F));
      }
      __syncthreads();
      if (tid < nr) {
        float s = 0.0f;
        for (int p = b; p < e; p++) s = norm_add(s, lds[p - off]);
        unscaled = !norm_scales(s);
        const float scale = norm_scale(s);
        for (int p = b; p < e; p++) lds[p - off] = scale;
      }
      __syncthreads();
      for (int q = (a_lo >> 2) + tid; q < (a_hi >> 2); q += kNormThreads) {
        const float4 v = j.val_in ? reinterpret_cast<const float4 *>(j.val_in)[q] : make_float4(1.0f, 1.0f, 1.0f, 1.0f);
        const float4 sc = *reinterpret_cast<const float4 *>(&lds[(q << 2) - off]);
        reinterpret_cast<float4 *>(j.val_out)[q] =
            make_float4(norm_apply(v.x, sc.x), norm_apply(v.y, sc.y), norm_apply(v.z, sc.z), norm_apply(v.w, sc.w));
      }
      for (int i = tid; i < n_edge; i += kNormThreads) {
        const int p = i < n_head ? base + i : a_hi + (i - n_head);
        j.val_out[p] = norm_apply(j.val_in ? j.val_in[p] : 1.0f, lds[p - off]);
      }
      __syncthreads();  // (the next run's squares go where these scales are)
    } else if (tid < nr) {
      float s = 0.0f;
      for (int p = b; p < e; p++) {
        const float v = j.val_in ? j.val_in[p] : 1.0f;
        s = norm_add(s, norm_square(v, norm_keeps(j.feat[p], fielded ? j.field[p] : 0, j.n_feats, F)));
      }
      unscaled = !norm_scales(s);
      const float scale = norm_scale(s);
      for (int p = b; p < e; p++) j.val_out[p] = norm_apply(j.val_in ? j.val_in[p] : 1.0f, scale);
    }
    const unsigned long long mask = __ballot(unscaled);
    if ((tid & 63) == 0 && mask)
      __hip_atomic_fetch_add(j.unscaled, static_cast<unsigned long long>(__popcll(mask)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace ftrl_dev
