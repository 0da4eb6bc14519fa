// kernels_rows.h -- resident rows (include/ffm_engine.h "Resident rows"): the kernel of a row cutter, and the one
// that mirrors a parsed slot's row_ptr to the host.  The cutter's appends
// rows [r0, r1) of a CSR block that already lies in HBM (a text parser's slot) to the block a cutter is assembling,
// also in HBM: the entries of field / feat / val and the labels are copied, row_ptr is rebased to the destination's
// running entry count.  Its launch and the ring of block buffers are host code: engine_rows.h.
#pragma once
#include <cstdint>

namespace ftrl_dev {

// Everything that sizes the kernel comes from the HOST, which read it from the page-locked mirror of the source's
// row_ptr (ffm_engine_textparse_wait_rows): the kernel reads no count from memory.  n_entries and n_rows are what
// the destination still has room for at most (the host refuses a take beyond the capacities before it launches;
// cap_entries / cap_rows guard every store once more).
struct RowTakeJob {
  const int *src_row_ptr, *src_field, *src_feat, *src_label;  // the source block's arrays (whole)
  const float *src_val;
  int *dst_row_ptr, *dst_field, *dst_feat, *dst_label;  // the destination buffers (whole, 16-byte aligned)
  float *dst_val;
  unsigned r0, n_rows;     // source rows [r0, r0 + n_rows)
  unsigned e0, n_entries;  // source entries [e0, e0 + n_entries): row_ptr[r0] .. row_ptr[r0 + n_rows]
  unsigned dst_row, dst_entry;  // where they go: the destination's running row and entry counts
  unsigned cap_rows, cap_entries;  // the destination's capacities
};

// n words from s to d over the grid: d's ragged head singly, then 16 bytes per lane -- loaded as one vector where s
// is aligned there as well, as four words where the two are not aligned to each other -- and the ragged tail singly.
// Nothing is stored at or past d_end.
__device__ __forceinline__ void rows_copy_words(const int *__restrict__ s, int *__restrict__ d, unsigned n, const int *d_end, unsigned tid,
                                                unsigned stride) {
  if (d >= d_end) return;
  const unsigned room = static_cast<unsigned>(d_end - d);
  if (n > room) n = room;
  unsigned head = (4u - (static_cast<unsigned>(reinterpret_cast<uintptr_t>(d) >> 2) & 3u)) & 3u;
  if (head > n) head = n;
  if (tid < head) d[tid] = s[tid];
  s += head;
  d += head;
  const unsigned m = n - head, n4 = m >> 2;
  if ((reinterpret_cast<uintptr_t>(s) & 15u) == 0) {
    for (unsigned i = tid; i < n4; i += stride) reinterpret_cast<int4 *>(d)[i] = reinterpret_cast<const int4 *>(s)[i];
  } else {
    for (unsigned i = tid; i < n4; i += stride) {
      const unsigned p = i << 2;
      reinterpret_cast<int4 *>(d)[i] = make_int4(s[p], s[p + 1], s[p + 2], s[p + 3]);
    }
  }
  if (tid < (m & 3u)) d[(n4 << 2) + tid] = s[(n4 << 2) + tid];
}

// No workgroup waits for another: every lane copies its own stride of every array and is done.
__global__ __launch_bounds__(256) void rows_take_kernel(RowTakeJob job) {
  const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  rows_copy_words(job.src_field + job.e0, job.dst_field + job.dst_entry, job.n_entries, job.dst_field + job.cap_entries, tid, stride);
  rows_copy_words(job.src_feat + job.e0, job.dst_feat + job.dst_entry, job.n_entries, job.dst_feat + job.cap_entries, tid, stride);
  rows_copy_words(reinterpret_cast<const int *>(job.src_val) + job.e0, reinterpret_cast<int *>(job.dst_val) + job.dst_entry, job.n_entries,
                  reinterpret_cast<const int *>(job.dst_val) + job.cap_entries, tid, stride);
  rows_copy_words(job.src_label + job.r0, job.dst_label + job.dst_row, job.n_rows, job.dst_label + job.cap_rows, tid, stride);
  // row_ptr, rebased: the destination's row dst_row + i ends where the source's row r0 + i does, moved by dst_entry - e0
  // (row_ptr has cap_rows + 1 elements)
  const unsigned room = job.cap_rows > job.dst_row ? job.cap_rows - job.dst_row : 0u;
  const unsigned n = job.n_rows < room ? job.n_rows : room;
  const int shift = static_cast<int>(job.dst_entry) - static_cast<int>(job.e0);
  for (unsigned i = tid; i < n; i += stride) job.dst_row_ptr[job.dst_row + 1 + i] = job.src_row_ptr[job.r0 + 1 + i] + shift;
  if (tid == 0 && job.dst_row == 0) job.dst_row_ptr[0] = 0;
}

// The page-locked host mirror of a parsed slot's row_ptr (ffm_engine_textparse_wait_rows): row_ptr[0 .. n_rows] to
// device-mapped host memory, 4 bytes per row -- the one place that reads the row count on the device (the slot's
// counters, kernels_text.h: TC_ROWS), so that nothing but the rows that exist crosses PCIe; at most cap + 1 words
// (a block that overflowed has no valid arrays, and the host does not read its mirror).  Launched on the parser's
// stream behind the parse, ahead of the slot's event.
__global__ __launch_bounds__(256) void rows_mirror_kernel(const int *__restrict__ row_ptr, const long long *__restrict__ counters, int *__restrict__ dst,
                                                          unsigned cap) {
  const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  const long long rows = counters[2];  // TC_ROWS
  const unsigned n = (rows < 0 ? 0u : rows > static_cast<long long>(cap) ? cap : static_cast<unsigned>(rows)) + 1u;
  for (unsigned i = tid; i < n; i += stride) dst[i] = row_ptr[i];
  __threadfence_system();
}

}  // namespace ftrl_dev
