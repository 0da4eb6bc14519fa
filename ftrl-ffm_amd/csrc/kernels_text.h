// kernels_text.h -- libffm / libsvm text to a CSR block on the device (include/ffm_engine.h "Text blocks"; the grammar,
// shared with the host bit for bit: text_parse.h).
//
// Bytes of whole lines in HBM go in, the block parse_csr_range (host/csr_reader.cpp) would produce comes out.  Six
// small launches on one stream; no workgroup ever waits for another (no grid barrier, no spin, no look-back): what
// has to cross workgroups -- a count, a scan, a write -- crosses a launch boundary.
//   1. text_count_newlines_kernel   a workgroup per kTextScanBytes of text: its number of '\n'
//   2. text_scan_kernel<0>          ONE workgroup: those counts to exclusive offsets; n_lines; the counters reset
//   3. text_line_starts_kernel      the same tiles again: line_start[k + 1] = position behind the k-th '\n'
//   4. text_lines_kernel<false>     a workgroup per kTextLineTile lines, a WAVE per line: (is_row, kept entries, slow)
//                                   per line, their sums per tile, n_slow and the first slow line's offset
//   5. text_scan_kernel<1>          ONE workgroup: the tiles' sums to exclusive offsets; n_rows, nnz, overflow
//   6. text_lines_kernel<true>      the lines parsed again, now with their row number and their entries' offset known:
//                                   row_ptr, label, field, feat, val.  Not run past its first line when the block has a
//                                   slow line or overflows (the arrays are then not valid anyway).
// Parsing twice costs less than any scheme that keeps per-token scratch between the passes.
//
// A line in a wave: the lanes take the line 16 bytes each, kTextTileBytes = 1024 per step, as aligned 16-byte loads
// (the text buffer is padded so that the load holding the last byte stays inside it; bytes outside [line begin,
// line end) are masked before anything is compared).  A byte starts a token when it is no blank and the byte before
// it is one (or the line begins there): a 16-bit mask per lane, the byte before a lane's first from the lane below
// (from the previous step for lane 0).  Tokens are ranked by popcount and a wave scan, token 0 is the label, and
// every lane parses the tokens that START in its 16 bytes with the shared grammar functions, reading on through
// the text however far the token goes -- so a token may straddle lanes and steps, and a line may hold any number
// of tokens.  At most 8 tokens start in 16 bytes, so the write pass keeps a lane's entries in registers (statically
// indexed) between the parse and the scan of the kept ones that places them.
//
// Bounds: every store is guarded by the capacity of its array; every load of text lies in [0, round16(n_bytes)).
#pragma once
#include "text_parse.h"

namespace ftrl_dev {

constexpr int kTextThreads = 256;
constexpr int kTextTileBytes = 1024;   // bytes of a line one wave step reads (64 lanes x 16)
constexpr int kTextScanBytes = 4096;   // bytes of text per workgroup of the newline count (256 threads x 16)
constexpr int kTextLineTile = 64;      // lines per workgroup of the line passes (16 per wave)
constexpr int kTextScanChunk = 256;    // elements the one-workgroup scans take per step

// counters of one parse (int64 each)
enum { TC_LINES, TC_NEWLINES, TC_ROWS, TC_NNZ, TC_SLOW, TC_FIRST_SLOW, TC_OVERFLOW, TC_COUNT };

struct TextArgs {
  const char *text;          // [round16(max_bytes) + 16]
  int32_t n_bytes, has_field;
  int32_t max_rows, max_nnz;
  int32_t cap_lines;         // entries of line_start; info holds cap_lines - 1
  int32_t cap_btiles, cap_ltiles;
  int32_t *line_start;       // [cap_lines] line i begins here
  uint32_t *info;            // per line: kept << 2 | is_row << 1 | slow
  uint32_t *btile;           // [cap_btiles] newlines per byte tile, then their exclusive scan
  uint32_t *ltile_rows, *ltile_nnz;  // [cap_ltiles] per line tile, then their exclusive scans
  long long *counters;       // [TC_COUNT]
  int32_t *row_ptr, *field, *feat, *label;
  float *val;
};

__device__ __forceinline__ int text_wave_excl(int x, int lane) {  // exclusive prefix sum over the wave's 64 lanes
  int s = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(s, d, 64);
    if (lane >= d) s += y;
  }
  return s - x;
}

// The 16 bytes at text + at (at % 16 == 0) as a mask of the bytes equal to `what`; only positions below `limit` count.
__device__ __forceinline__ unsigned text_eq_mask(const uint4 w, unsigned what, int at, int limit) {
  const unsigned words[4] = {w.x, w.y, w.z, w.w};
  unsigned m = 0;
#pragma unroll
  for (int k = 0; k < 16; k++) m |= (((words[k >> 2] >> (8 * (k & 3))) & 0xffu) == what ? 1u : 0u) << k;
  const int n = limit - at;
  return n >= 16 ? m : n <= 0 ? 0u : (m & ((1u << n) - 1u));
}

__global__ __launch_bounds__(kTextThreads) void text_count_newlines_kernel(TextArgs a) {
  __shared__ int part[kTextThreads / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n_tiles = (a.n_bytes + kTextScanBytes - 1) / kTextScanBytes;
  for (int t = blockIdx.x; t < n_tiles && t < a.cap_btiles; t += gridDim.x) {
    const int at = t * kTextScanBytes + static_cast<int>(threadIdx.x) * 16;
    int c = 0;
    if (at < a.n_bytes) c = __popc(text_eq_mask(*reinterpret_cast<const uint4 *>(a.text + at), '\n', at, a.n_bytes));
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d, 64);
    if (lane == 0) part[wv] = c;
    __syncthreads();
    if (threadIdx.x == 0) a.btile[t] = static_cast<uint32_t>(part[0] + part[1] + part[2] + part[3]);
    __syncthreads();
  }
}

// One workgroup.  WHICH 0: btile[0 .. byte tiles) to exclusive offsets, n_newlines, n_lines, line_start[0], and the
// counters of the line passes reset.  WHICH 1: ltile_rows / ltile_nnz[0 .. line tiles) to exclusive offsets, n_rows,
// nnz, overflow, and the last row_ptr.
template <int WHICH>
__global__ __launch_bounds__(kTextScanChunk) void text_scan_kernel(TextArgs a) {
  __shared__ unsigned long long wsum[2][kTextScanChunk / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int n;
  if (WHICH == 0) {
    n = (a.n_bytes + kTextScanBytes - 1) / kTextScanBytes;
    if (n > a.cap_btiles) n = a.cap_btiles;
  } else {
    const long long n_lines = a.counters[TC_LINES];
    n = static_cast<int>((n_lines + kTextLineTile - 1) / kTextLineTile);
    if (n > a.cap_ltiles) n = a.cap_ltiles;
  }
  unsigned long long carry0 = 0, carry1 = 0;
  for (int i0 = 0; i0 < n; i0 += kTextScanChunk) {
    const int i = i0 + static_cast<int>(threadIdx.x);
    const int x0 = i < n ? static_cast<int>(WHICH == 0 ? a.btile[i] : a.ltile_rows[i]) : 0;
    const int x1 = (WHICH == 1 && i < n) ? static_cast<int>(a.ltile_nnz[i]) : 0;
    const int e0 = text_wave_excl(x0, lane), e1 = WHICH == 1 ? text_wave_excl(x1, lane) : 0;
    if (lane == 63) {
      wsum[0][wv] = static_cast<unsigned>(e0 + x0);
      wsum[1][wv] = static_cast<unsigned>(e1 + x1);
    }
    __syncthreads();
    unsigned long long b0 = carry0, b1 = carry1, t0 = 0, t1 = 0;
#pragma unroll
    for (int w = 0; w < kTextScanChunk / 64; w++) {
      if (w < wv) {
        b0 += wsum[0][w];
        b1 += wsum[1][w];
      }
      t0 += wsum[0][w];
      t1 += wsum[1][w];
    }
    if (i < n) {
      if (WHICH == 0) a.btile[i] = static_cast<uint32_t>(b0 + static_cast<unsigned>(e0));
      else {
        a.ltile_rows[i] = static_cast<uint32_t>(b0 + static_cast<unsigned>(e0));
        a.ltile_nnz[i] = static_cast<uint32_t>(b1 + static_cast<unsigned>(e1));
      }
    }
    carry0 += t0;
    carry1 += t1;
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  if (WHICH == 0) {
    const long long last_open = (a.n_bytes > 0 && a.text[a.n_bytes - 1] != '\n') ? 1 : 0;
    a.counters[TC_NEWLINES] = static_cast<long long>(carry0);
    a.counters[TC_LINES] = static_cast<long long>(carry0) + last_open;
    a.counters[TC_SLOW] = 0;
    a.counters[TC_FIRST_SLOW] = 0x7fffffffffffffffll;
    if (a.cap_lines > 0) a.line_start[0] = 0;
  } else {
    const long long rows = static_cast<long long>(carry0), nnz = static_cast<long long>(carry1);
    const int over = (rows > a.max_rows || nnz > a.max_nnz) ? 1 : 0;
    a.counters[TC_ROWS] = rows;
    a.counters[TC_NNZ] = nnz;
    a.counters[TC_OVERFLOW] = over;
    if (!over) a.row_ptr[rows] = static_cast<int32_t>(nnz);  // (rows <= max_rows: row_ptr holds max_rows + 1)
  }
}

__global__ __launch_bounds__(kTextThreads) void text_line_starts_kernel(TextArgs a) {
  __shared__ int part[kTextThreads / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n_tiles = (a.n_bytes + kTextScanBytes - 1) / kTextScanBytes;
  for (int t = blockIdx.x; t < n_tiles && t < a.cap_btiles; t += gridDim.x) {
    const int at = t * kTextScanBytes + static_cast<int>(threadIdx.x) * 16;
    unsigned m = 0;
    if (at < a.n_bytes) m = text_eq_mask(*reinterpret_cast<const uint4 *>(a.text + at), '\n', at, a.n_bytes);
    const int c = __popc(m);
    const int ex = text_wave_excl(c, lane);
    if (lane == 63) part[wv] = ex + c;
    __syncthreads();
    unsigned k = a.btile[t] + static_cast<unsigned>(ex);
    for (int w = 0; w < wv; w++) k += static_cast<unsigned>(part[w]);
    while (m) {
      const int b = __ffs(m) - 1;
      m &= m - 1;
      k++;  // the k-th newline ends line k - 1: line k begins behind it
      if (k < static_cast<unsigned>(a.cap_lines)) a.line_start[k] = at + b + 1;
    }
    __syncthreads();
  }
}

// One line [lb, le) (le: its '\n' or the text's end) in one wave.  WRITE: the line is row `row`, its kept entries go
// to [ent, ent + kept).  Out, wave-uniform: is_row, kept, slow -- a slow line is no row and keeps nothing.
template <bool WRITE>
__device__ __forceinline__ void text_parse_line(const TextArgs &a, int lane, int lb, int le, int row, int ent, int &is_row, int &kept,
                                                int &slow) {
  is_row = 0;
  kept = 0;
  slow = 0;
  if (le - lb > ftrl_text::kMaxLine) {
    slow = 1;
    return;
  }
  const char *t = a.text;
  int stop = le;
  if (stop > lb && t[stop - 1] == '\r') stop--;
  const bool has_field = a.has_field != 0;
  int n_tok = 0, n_kept = 0;
  unsigned carry = 0;  // the last byte of the previous step was no blank
  bool bad = false;
  for (int a0 = lb & ~15; a0 < stop; a0 += kTextTileBytes) {
    const int ca = a0 + lane * 16;
    unsigned nb = 0;
    if (ca < stop) {
      const unsigned blank = text_eq_mask(*reinterpret_cast<const uint4 *>(t + ca), ' ', ca, stop);
      const int lo = lb - ca, hi = stop - ca;
      unsigned in = hi >= 16 ? 0xffffu : ((1u << hi) - 1u);
      if (lo > 0) in &= ~((1u << (lo > 16 ? 16 : lo)) - 1u);
      nb = ~blank & in;
    }
    unsigned below = __shfl_up(nb >> 15, 1, 64);
    if (lane == 0) below = carry;
    carry = __shfl(nb >> 15, 63, 64);
    unsigned m = nb & ~((nb << 1) | below) & 0xffffu;
    const int c = __popc(m);
    const int ex = text_wave_excl(c, lane);
    const int total = __shfl(ex + c, 63, 64);
    int r = n_tok + ex;
    unsigned keep = 0;
    int fld[8], ft[8];
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      fld[j] = 0;
      ft[j] = 0;
      v[j] = 0.0f;
      if (m) {
        const int q = ca + __ffs(m) - 1;
        m &= m - 1;
        if (r == 0) {
          int lab = 0;
          const bool ok = ftrl_text::parse_label(t, q, stop, lab);
          bad = bad || !ok;
          if (WRITE && ok && row >= 0 && row < a.max_rows) {
            a.label[row] = lab;
            a.row_ptr[row] = ent;
          }
        } else {
          const bool ok = ftrl_text::parse_entry(t, q, stop, has_field, fld[j], ft[j], v[j]);
          bad = bad || !ok;
          if (ok && v[j] != 0.0f) keep |= 1u << j;
        }
        r++;
      }
    }
    const int kc = __popc(keep);
    const int kex = text_wave_excl(kc, lane);
    if (WRITE) {
      int o = ent + n_kept + kex;
#pragma unroll
      for (int j = 0; j < 8; j++)
        if ((keep >> j) & 1u) {
          if (o >= 0 && o < a.max_nnz) {
            a.field[o] = fld[j];
            a.feat[o] = ft[j];
            a.val[o] = v[j];
          }
          o++;
        }
    }
    n_tok += total;
    n_kept += __shfl(kex + kc, 63, 64);
  }
  if (__ballot(bad) != 0ull) {
    slow = 1;
    return;
  }
  is_row = n_tok > 0 ? 1 : 0;
  kept = n_kept;
}

template <bool WRITE>
__global__ __launch_bounds__(kTextThreads) void text_lines_kernel(TextArgs a) {
  __shared__ int s_row[kTextLineTile], s_ent[kTextLineTile];
  __shared__ int s_sum[2][kTextThreads / 64];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const long long n_lines_ll = a.counters[TC_LINES];
  const int n_newlines = static_cast<int>(a.counters[TC_NEWLINES]);
  int n_lines = static_cast<int>(n_lines_ll);
  if (n_lines > a.cap_lines - 1) n_lines = a.cap_lines - 1;
  if (WRITE && (a.counters[TC_SLOW] != 0 || a.counters[TC_OVERFLOW] != 0)) return;  // (the arrays are not valid anyway)
  int n_tiles = (n_lines + kTextLineTile - 1) / kTextLineTile;
  if (n_tiles > a.cap_ltiles) n_tiles = a.cap_ltiles;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int l0 = tile * kTextLineTile;
    if (WRITE) {
      if (wv == 0) {  // line = lane: the tile's lines to row numbers and entry offsets
        const int l = l0 + lane;
        const unsigned inf = l < n_lines ? a.info[l] : 0u;
        const int isr = static_cast<int>((inf >> 1) & 1u), k = static_cast<int>(inf >> 2);
        s_row[lane] = static_cast<int>(a.ltile_rows[tile]) + text_wave_excl(isr, lane);
        s_ent[lane] = static_cast<int>(a.ltile_nnz[tile]) + text_wave_excl(k, lane);
      }
      __syncthreads();
    }
    int rows = 0, nnz = 0, n_slow = 0, first_slow = 0x7fffffff;
    for (int j = wv; j < kTextLineTile; j += kTextThreads / 64) {
      const int l = l0 + j;
      if (l >= n_lines) break;
      const int lb = a.line_start[l];
      const int le = l < n_newlines ? a.line_start[l + 1] - 1 : a.n_bytes;
      if (lb < 0 || le < lb || le > a.n_bytes) continue;  // (cannot be: line_start is ascending inside the text)
      int is_row, kept, slow;
      text_parse_line<WRITE>(a, lane, lb, le, WRITE ? s_row[j] : 0, WRITE ? s_ent[j] : 0, is_row, kept, slow);
      if (!WRITE) {
        if (lane == 0) a.info[l] = (static_cast<unsigned>(kept) << 2) | (static_cast<unsigned>(is_row) << 1) | static_cast<unsigned>(slow);
        rows += is_row;
        nnz += kept;
        if (slow && n_slow++ == 0) first_slow = lb;
      }
    }
    if (!WRITE) {
      if (lane == 0) {
        s_sum[0][wv] = rows;
        s_sum[1][wv] = nnz;
        if (n_slow) {
          atomicAdd(reinterpret_cast<unsigned long long *>(a.counters + TC_SLOW), static_cast<unsigned long long>(n_slow));
          atomicMin(a.counters + TC_FIRST_SLOW, static_cast<long long>(first_slow));
        }
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        a.ltile_rows[tile] = static_cast<uint32_t>(s_sum[0][0] + s_sum[0][1] + s_sum[0][2] + s_sum[0][3]);
        a.ltile_nnz[tile] = static_cast<uint32_t>(s_sum[1][0] + s_sum[1][1] + s_sum[1][2] + s_sum[1][3]);
      }
    }
    __syncthreads();
  }
}

}  // namespace ftrl_dev
