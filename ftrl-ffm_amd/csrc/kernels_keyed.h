// kernels_keyed.h -- keyed capture and its reduction: the per-key AUC (GAUC) behind
// ffm_engine_metrics_*_keyed (include/ffm_engine.h "Metrics", keyed capture).
//
// Capture (keyed_capture_kernel, one launch per labelled block and channel): one 64-bit word per row,
//   word = key << 32 | (bits of p) << 1 | class,      p = sigmoid_ref(logit), p in [0, 1] so its bits
// are at most 0x3F800000 and bit 31 of the word is always 0.  Ascending words order a key's rows by p,
// negatives first inside a tie: sorting the words alone is the whole ranking.
// Lane mapping: kKeyedSub = 8 lanes per row.  A row of the headline shape has about 39 entries in field
// order; a lane per row would walk them one dependent load after another with 64 rows' addresses 156
// bytes apart (every load of a wave 64 cache lines), eight lanes read 32 contiguous bytes per row and
// step, end after five steps at the most, and after ONE when the key field comes first.  The first
// matching entry in row order is the minimum of the lanes' first matches (three shuffles).
// Slots are reserved by one 64-bit atomic per wave (ballot + popcount, as metric_hist_kernel does),
// only slots below the capacity are stored; the NaN / unkeyed / overflow counters take one integer
// atomic per wave each.
//
// Read, all on the engine's stream, every kernel free of waits on other workgroups (no look-back, no
// spin, no grid barrier: what has to be known across workgroups is a launch boundary):
//   sort   LSD radix sort, 8 bits per pass: per-workgroup digit histogram -> exclusive scan of
//          [digit][workgroup] -> stable scatter.  The passes whose digit is constant are skipped by the
//          host: bit 31, and the bits above the key's width.
//   scan   every scan is three launches: tile sums, one workgroup over the sums, apply.
//   rank   over the sorted words the scan of (negatives so far, negatives before the current key's
//          start, negatives before the current (key, p) run's start, key starts so far) -- an
//          associative operator, RankState below.  A positive at i adds
//          2 * (neg[i] - neg[keystart]) - (neg[i] - neg[runstart]) = 2 * #{smaller neg} + #{equal neg}
//          to its key's U2; P, N, U2 go into the per-key table with 64-bit integer atomics (exact,
//          order-free), a thread first adding up what its own consecutive rows give one key.
#pragma once
#include "engine_types.h"
#include "ftrl_math.h"

namespace ftrl_dev {

constexpr int kKeyedThreads = 256;
constexpr int kKeyedSub = 8;                                  // lanes per row of the capture kernel
constexpr int kKeyedRowsPerWg = kKeyedThreads / kKeyedSub;    // 32
constexpr int kKeyedItems = 8;                                // consecutive words per thread of the rank pass
constexpr int kKeyedTile = kKeyedThreads * kKeyedItems;       // 2048: the rank pass's scan tile
constexpr int kKeyedScanItems = 8;                            // the histogram scan: counters per thread
constexpr int kKeyedScanTile = kKeyedThreads * kKeyedScanItems;
constexpr unsigned kKeyedNone = 0xffffffffu;

// counters of one channel: rows that asked for a slot (may pass the capacity), NaN, unkeyed, overflow
enum { KEYED_N_ASKED = 0, KEYED_N_NAN = 1, KEYED_N_UNKEYED = 2, KEYED_N_OVERFLOW = 3, KEYED_COUNTERS = 4 };

__device__ __forceinline__ void keyed_wave_count(unsigned long long *counter, bool mine, int lane) {
  const unsigned long long mask = __ballot(mine);
  if (mask != 0ull && lane == __ffsll(mask) - 1)
    __hip_atomic_fetch_add(counter, static_cast<unsigned long long>(__popcll(mask)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kKeyedThreads) void keyed_capture_kernel(Rows rows, int n_feats, int key_field, const float *score,
                                                                      int is_prob, unsigned long long *words,
                                                                      unsigned long long capacity, unsigned long long *counters) {
  const int lane = threadIdx.x & 63, sub = threadIdx.x & (kKeyedSub - 1);
  const int r = blockIdx.x * kKeyedRowsPerWg + threadIdx.x / kKeyedSub;
  const bool live = r < rows.n_rows;
  // this lane's first entry (row order) of the key field with an id the model holds: position << 32 | id
  unsigned long long best = ~0ull;
  if (live && rows.field) {
    const int end = rows.row_ptr[r + 1];
    for (int j = rows.row_ptr[r] + sub; j < end; j += kKeyedSub) {
      if (rows.field[j] != key_field) continue;
      const int f = rows.feat[j];
      if (static_cast<unsigned>(f) < static_cast<unsigned>(n_feats)) {
        best = static_cast<unsigned long long>(static_cast<unsigned>(j)) << 32 | static_cast<unsigned>(f);
        break;
      }
    }
  }
  // (every lane of the wave is here again: the row's first match is the smallest of its eight lanes')
  for (int off = 1; off < kKeyedSub; off <<= 1) {
    const unsigned long long other = __shfl_xor(best, off);
    best = other < best ? other : best;
  }
  const bool head = live && sub == 0;  // one lane speaks for the row
  float p = 0.0f;
  int cls = 0;
  if (head) {
    const float s = score[r];
    p = is_prob ? s : sigmoid_ref(s);
    cls = rows.label[r] > 0 ? 1 : 0;
  }
  const bool is_nan = head && p != p;
  const bool unkeyed = head && !is_nan && best == ~0ull;
  const bool wants = head && !is_nan && !unkeyed;
  keyed_wave_count(counters + KEYED_N_NAN, is_nan, lane);
  keyed_wave_count(counters + KEYED_N_UNKEYED, unkeyed, lane);
  const unsigned long long mask = __ballot(wants);
  unsigned long long base = 0ull;
  if (mask != 0ull) {
    const int first = __ffsll(mask) - 1;
    if (lane == first)
      base = __hip_atomic_fetch_add(counters + KEYED_N_ASKED, static_cast<unsigned long long>(__popcll(mask)), __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
    base = __shfl(base, first);
  }
  const unsigned long long slot = base + static_cast<unsigned long long>(__popcll(mask & ((1ull << lane) - 1ull)));
  const bool stored = wants && slot < capacity;
  if (stored)  // (the & keeps a sign bit no sigmoid returns out of the key)
    words[slot] = (best & 0xffffffffull) << 32 | static_cast<unsigned long long>(__float_as_uint(p) & 0x7fffffffu) << 1 |
                  static_cast<unsigned long long>(cls);
  keyed_wave_count(counters + KEYED_N_OVERFLOW, wants && !stored, lane);
}

// ---- a workgroup's exclusive scan of one value per thread, for any associative operator ------------
// (not commutative for RankState: op(earlier, later)).  `wave_tot` is kKeyedThreads / 64 values of LDS.

struct SumU32 {
  typedef unsigned T;
  static __device__ __forceinline__ T identity() { return 0u; }
  static __device__ __forceinline__ T op(T a, T b) { return a + b; }
  static __device__ __forceinline__ T up(T v, int off) { return __shfl_up(v, off); }
};

// neg: negatives in the segment; key / run: negatives of the segment before its LAST key start / run
// start, kKeyedNone when it holds none; starts: key starts in the segment.
struct RankState { unsigned neg, key, run, starts; };
struct RankOp {
  typedef RankState T;
  static __device__ __forceinline__ T identity() { return RankState{0u, kKeyedNone, kKeyedNone, 0u}; }
  static __device__ __forceinline__ T op(const T &a, const T &b) {
    return RankState{a.neg + b.neg, b.key != kKeyedNone ? a.neg + b.key : a.key, b.run != kKeyedNone ? a.neg + b.run : a.run,
                     a.starts + b.starts};
  }
  static __device__ __forceinline__ T up(const T &v, int off) {
    return RankState{__shfl_up(v.neg, off), __shfl_up(v.key, off), __shfl_up(v.run, off), __shfl_up(v.starts, off)};
  }
};

// Returns op(everything before this thread); *total = op(all threads), the same in every thread.
template <class Op>
__device__ __forceinline__ typename Op::T keyed_block_exclusive(typename Op::T v, typename Op::T *wave_tot, typename Op::T *total) {
  typedef typename Op::T T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T inc = v;
  for (int off = 1; off < 64; off <<= 1) {
    const T other = Op::up(inc, off);
    if (lane >= off) inc = Op::op(other, inc);
  }
  T exc = Op::up(inc, 1);
  if (lane == 0) exc = Op::identity();
  __syncthreads();  // (wave_tot may still be read from the call before)
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  T before = Op::identity(), all = Op::identity();
  for (int w = 0; w < kKeyedThreads / 64; w++) {
    if (w == wave) before = all;
    all = Op::op(all, wave_tot[w]);
  }
  *total = all;
  return Op::op(before, exc);
}

// ---- the three launches of an exclusive scan of 32-bit counters, in place ---------------------------

__global__ __launch_bounds__(kKeyedThreads) void keyed_scan_sums_kernel(const unsigned *a, unsigned n, unsigned *sums) {
  __shared__ unsigned wave_tot[kKeyedThreads / 64];
  const unsigned i0 = blockIdx.x * static_cast<unsigned>(kKeyedScanTile) + threadIdx.x * kKeyedScanItems;
  unsigned s = 0u;
  for (int j = 0; j < kKeyedScanItems; j++)
    if (i0 + j < n) s += a[i0 + j];
  unsigned total;
  (void)keyed_block_exclusive<SumU32>(s, wave_tot, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// One workgroup: sums[0 .. n_tiles) -> their exclusive scan, in place; a thread takes a run of them.
template <class Op>
__global__ __launch_bounds__(kKeyedThreads) void keyed_scan_top_kernel(typename Op::T *sums, unsigned n_tiles) {
  typedef typename Op::T T;
  __shared__ T wave_tot[kKeyedThreads / 64];
  const unsigned per = (n_tiles + kKeyedThreads - 1) / kKeyedThreads;
  const unsigned lo = min(threadIdx.x * per, n_tiles), hi = min(lo + per, n_tiles);
  T mine = Op::identity();
  for (unsigned t = lo; t < hi; t++) mine = Op::op(mine, sums[t]);
  T total;
  T run = keyed_block_exclusive<Op>(mine, wave_tot, &total);
  for (unsigned t = lo; t < hi; t++) {
    const T v = sums[t];
    sums[t] = run;
    run = Op::op(run, v);
  }
}

__global__ __launch_bounds__(kKeyedThreads) void keyed_scan_apply_kernel(unsigned *a, unsigned n, const unsigned *sums) {
  __shared__ unsigned wave_tot[kKeyedThreads / 64];
  const unsigned i0 = blockIdx.x * static_cast<unsigned>(kKeyedScanTile) + threadIdx.x * kKeyedScanItems;
  unsigned v[kKeyedScanItems], s = 0u;
  for (int j = 0; j < kKeyedScanItems; j++) {
    v[j] = i0 + j < n ? a[i0 + j] : 0u;
    s += v[j];
  }
  unsigned total;
  unsigned run = sums[blockIdx.x] + keyed_block_exclusive<SumU32>(s, wave_tot, &total);
  for (int j = 0; j < kKeyedScanItems; j++) {
    if (i0 + j < n) a[i0 + j] = run;
    run += v[j];
  }
}

// ---- the sort's two kernels: workgroup w owns words [w * chunk, min(n, (w + 1) * chunk)) --------------
// chunk is a multiple of kKeyedThreads; hist is [256][n_wg].

__global__ __launch_bounds__(kKeyedThreads) void keyed_sort_hist_kernel(const unsigned long long *in, unsigned n, unsigned chunk,
                                                                        int shift, unsigned dmask, unsigned *hist) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const unsigned long long begin = static_cast<unsigned long long>(blockIdx.x) * chunk;
  const unsigned long long end = min(begin + chunk, static_cast<unsigned long long>(n));
  for (unsigned long long i = begin + threadIdx.x; i < end; i += kKeyedThreads)
    atomicAdd(&h[static_cast<unsigned>(in[i] >> shift) & dmask], 1u);
  __syncthreads();
  hist[static_cast<size_t>(threadIdx.x) * gridDim.x + blockIdx.x] = h[threadIdx.x];
}

// offs: hist after its exclusive scan = where this workgroup's first word of every digit goes.  Stable:
// a sub-tile of 256 words in thread order, inside it the waves in order, inside a wave the lanes in order.
__global__ __launch_bounds__(kKeyedThreads) void keyed_sort_scatter_kernel(const unsigned long long *in, unsigned long long *out,
                                                                           unsigned n, unsigned chunk, int shift, unsigned dmask,
                                                                           const unsigned *offs) {
  constexpr int kWaves = kKeyedThreads / 64;
  __shared__ unsigned base[256];
  __shared__ unsigned wcnt[kWaves][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  base[threadIdx.x] = offs[static_cast<size_t>(threadIdx.x) * gridDim.x + blockIdx.x];
  const unsigned long long begin = static_cast<unsigned long long>(blockIdx.x) * chunk;
  const unsigned long long end = min(begin + chunk, static_cast<unsigned long long>(n));
  for (unsigned long long sub = begin; sub < end; sub += kKeyedThreads) {  // (uniform over the workgroup)
    const unsigned long long i = sub + threadIdx.x;
    const bool live = i < end;
    const unsigned long long w = live ? in[i] : 0ull;
    const unsigned d = static_cast<unsigned>(w >> shift) & dmask;
    for (int u = 0; u < kWaves; u++) wcnt[u][threadIdx.x] = 0u;
    __syncthreads();
    // the lanes of this wave that carry the same digit
    unsigned long long same = __ballot(live);
    for (int b = 0; b < 8; b++) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bal = __ballot(bit);
      same &= bit ? bal : ~bal;
    }
    const unsigned rank = static_cast<unsigned>(__popcll(same & ((1ull << lane) - 1ull)));
    if (live && rank == 0u) wcnt[wave][d] = static_cast<unsigned>(__popcll(same));
    __syncthreads();
    if (live) {
      unsigned pos = base[d] + rank;
      for (int u = 0; u < wave; u++) pos += wcnt[u][d];
      if (pos < n) out[pos] = w;  // (always: the histogram counted these same words)
    }
    __syncthreads();
    unsigned add = 0u;
    for (int u = 0; u < kWaves; u++) add += wcnt[u][threadIdx.x];
    base[threadIdx.x] += add;
  }
}

// ---- the rank pass -----------------------------------------------------------------------------------

// The state of word i alone, given the word before it (i > 0).
__device__ __forceinline__ RankState keyed_leaf(unsigned long long w, unsigned long long prev, bool first) {
  const bool key_start = first || (w >> 32) != (prev >> 32);
  const bool run_start = first || (w >> 1) != (prev >> 1);
  return RankState{(w & 1ull) ? 0u : 1u, key_start ? 0u : kKeyedNone, run_start ? 0u : kKeyedNone, key_start ? 1u : 0u};
}

__global__ __launch_bounds__(kKeyedThreads) void keyed_rank_sums_kernel(const unsigned long long *words, unsigned n, RankState *sums) {
  __shared__ RankState wave_tot[kKeyedThreads / 64];
  const unsigned long long i0 = static_cast<unsigned long long>(blockIdx.x) * kKeyedTile + threadIdx.x * kKeyedItems;
  RankState s = RankOp::identity();
  unsigned long long prev = i0 > 0 && i0 < n ? words[i0 - 1] : 0ull;
  for (int j = 0; j < kKeyedItems; j++) {
    if (i0 + j >= n) break;
    const unsigned long long w = words[i0 + j];
    s = RankOp::op(s, keyed_leaf(w, prev, i0 + j == 0));
    prev = w;
  }
  RankState total;
  (void)keyed_block_exclusive<RankOp>(s, wave_tot, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums: the tiles' states after keyed_scan_top_kernel<RankOp> (exclusive).  tab_key[g] / tab[3 * g + {0, 1, 2}]
// = key / P, N, U2 of the g-th key in ascending order; n_tab entries (every key start below it is in range
// whenever n_tab >= min(n, key range): the host sizes it so).
__global__ __launch_bounds__(kKeyedThreads) void keyed_rank_apply_kernel(const unsigned long long *words, unsigned n,
                                                                         const RankState *sums, int *tab_key,
                                                                         unsigned long long *tab, unsigned n_tab,
                                                                         unsigned *n_keys_out) {
  __shared__ RankState wave_tot[kKeyedThreads / 64];
  const unsigned long long i0 = static_cast<unsigned long long>(blockIdx.x) * kKeyedTile + threadIdx.x * kKeyedItems;
  unsigned long long w[kKeyedItems];
  RankState leaf[kKeyedItems], s = RankOp::identity();
  unsigned long long prev = i0 > 0 && i0 < n ? words[i0 - 1] : 0ull;
  for (int j = 0; j < kKeyedItems; j++) {
    w[j] = i0 + j < n ? words[i0 + j] : 0ull;
    leaf[j] = i0 + j < n ? keyed_leaf(w[j], prev, i0 + j == 0) : RankOp::identity();
    s = RankOp::op(s, leaf[j]);
    prev = w[j];
  }
  RankState total;
  RankState run = RankOp::op(sums[blockIdx.x], keyed_block_exclusive<RankOp>(s, wave_tot, &total));
  // this thread's consecutive words: what they give one key is added up before it goes to the table
  unsigned g = kKeyedNone;
  unsigned long long add_p = 0ull, add_n = 0ull, add_u2 = 0ull;
  for (int j = 0; j < kKeyedItems; j++) {
    if (i0 + j >= n) break;
    const unsigned neg_before = run.neg;  // negatives in [0, i)
    run = RankOp::op(run, leaf[j]);       // inclusive: run.key / run.run are those of word i's key and run
    const unsigned gi = run.starts - 1u;
    if (i0 + j == n - 1u) *n_keys_out = run.starts;  // (the last word knows how many keys there are)
    if (gi != g) {
      if (g != kKeyedNone && g < n_tab) {
        if (add_p) __hip_atomic_fetch_add(tab + 3ull * g, add_p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (add_n) __hip_atomic_fetch_add(tab + 3ull * g + 1, add_n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (add_u2) __hip_atomic_fetch_add(tab + 3ull * g + 2, add_u2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      g = gi;
      add_p = add_n = add_u2 = 0ull;
    }
    if (leaf[j].starts && gi < n_tab) tab_key[gi] = static_cast<int>(w[j] >> 32);
    if (w[j] & 1ull) {
      add_p += 1ull;
      add_u2 += 2ull * (neg_before - run.key) - (neg_before - run.run);
    } else {
      add_n += 1ull;
    }
  }
  if (g != kKeyedNone && g < n_tab) {
    if (add_p) __hip_atomic_fetch_add(tab + 3ull * g, add_p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (add_n) __hip_atomic_fetch_add(tab + 3ull * g + 1, add_n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (add_u2) __hip_atomic_fetch_add(tab + 3ull * g + 2, add_u2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace ftrl_dev
