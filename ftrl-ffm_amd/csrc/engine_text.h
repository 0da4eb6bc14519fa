// engine_text.h -- text blocks (include/ffm_engine.h "Text blocks"), host side: a text parser's two slots -- each a
// padded text buffer, the line arrays and the CSR arrays in HBM, a page-locked image for pageable callers and a
// page-locked copy of the counters --, its stream, the six launches of kernels_text.h per parse, and the host twin
// (text_parse.h).  A parser touches nothing of an engine.  Part of engine.hip's translation unit (inside its
// extern "C" block).

struct ffm_textparse {
  int32_t has_field = 0, max_rows = 0, max_nnz = 0, device_id = 0;
  int64_t max_bytes = 0;
  hipStream_t stream = nullptr;
  struct Slot {
    char *d_text = nullptr;
    int32_t *d_line_start = nullptr;
    uint32_t *d_info = nullptr, *d_btile = nullptr, *d_ltile_rows = nullptr, *d_ltile_nnz = nullptr;
    long long *d_counters = nullptr;
    int32_t *d_row_ptr = nullptr, *d_field = nullptr, *d_feat = nullptr, *d_label = nullptr;
    float *d_val = nullptr;
    char *pinned = nullptr;          // [max_bytes] image of a pageable caller's text, made by the first such parse
    long long *h_counters = nullptr;  // page-locked [TC_COUNT]
    hipEvent_t ev_done = nullptr;
    bool in_flight = false;
    // the page-locked mirror of row_ptr (ffm_engine_textparse_wait_rows; made by the first such wait): whether this
    // slot's last parse copied into it, and how many rows of it a waited block vouches for (-1: none)
    int32_t *h_row_ptr = nullptr, *d_row_ptr_mirror = nullptr;  // (the second: the device's address of the first)
    bool mirror_copied = false;
    int64_t mirror_rows = -1;
  } slot[2];
  bool mirror_on = false;  // every parse copies its slot's row_ptr to the mirror, ahead of the slot's event
  int32_t cap_lines = 0, cap_btiles = 0, cap_ltiles = 0;
};

void ffm_engine_textparse_destroy(ffm_textparse *p) {
  if (!p) return;
  (void)hipSetDevice(p->device_id);
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  for (auto &s : p->slot) {
    void *dev[] = {s.d_text, s.d_line_start, s.d_info, s.d_btile, s.d_ltile_rows, s.d_ltile_nnz, s.d_counters,
                   s.d_row_ptr, s.d_field, s.d_feat, s.d_label, s.d_val};
    for (void *d : dev)
      if (d) (void)hipFree(d);
    if (s.pinned) (void)hipHostFree(s.pinned);
    if (s.h_counters) (void)hipHostFree(s.h_counters);
    if (s.h_row_ptr) (void)hipHostFree(s.h_row_ptr);
    if (s.ev_done) (void)hipEventDestroy(s.ev_done);
  }
  if (p->stream) (void)hipStreamDestroy(p->stream);
  delete p;
}

static int textparse_init(ffm_textparse *p) {
  HIP_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
  // the text padded to the vector width, and one vector more: the aligned 16-byte load that holds the last byte
  // (and the one of an empty text's neighbourhood) stays inside the allocation
  const size_t text_bytes = ((static_cast<size_t>(p->max_bytes) + 15) & ~static_cast<size_t>(15)) + 16;
  p->cap_lines = static_cast<int32_t>(p->max_bytes + 2);  // a text of B bytes has at most B lines: starts 0 .. B
  p->cap_btiles = static_cast<int32_t>((p->max_bytes + kTextScanBytes - 1) / kTextScanBytes) + 1;
  p->cap_ltiles = (p->cap_lines + kTextLineTile - 1) / kTextLineTile + 1;
  for (auto &s : p->slot) {
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s.d_text), text_bytes));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s.d_line_start), sizeof(int32_t) * static_cast<size_t>(p->cap_lines)));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s.d_info), sizeof(uint32_t) * static_cast<size_t>(p->cap_lines)));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s.d_btile), sizeof(uint32_t) * static_cast<size_t>(p->cap_btiles)));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s.d_ltile_rows), sizeof(uint32_t) * static_cast<size_t>(p->cap_ltiles)));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s.d_ltile_nnz), sizeof(uint32_t) * static_cast<size_t>(p->cap_ltiles)));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s.d_counters), sizeof(long long) * TC_COUNT));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s.d_row_ptr), sizeof(int32_t) * (static_cast<size_t>(p->max_rows) + 1)));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s.d_label), sizeof(int32_t) * static_cast<size_t>(std::max(p->max_rows, 1))));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s.d_field), sizeof(int32_t) * static_cast<size_t>(std::max(p->max_nnz, 1))));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s.d_feat), sizeof(int32_t) * static_cast<size_t>(std::max(p->max_nnz, 1))));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s.d_val), sizeof(float) * static_cast<size_t>(std::max(p->max_nnz, 1))));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&s.h_counters), sizeof(long long) * TC_COUNT, hipHostMallocPortable));
    HIP_TRY(hipEventCreateWithFlags(&s.ev_done, hipEventDisableTiming));
    HIP_TRY(hipMemsetAsync(s.d_text, 0, text_bytes, p->stream));
  }
  HIP_TRY(hipStreamSynchronize(p->stream));
  return FFM_OK;
}

int ffm_engine_textparse_create(int32_t has_field, int64_t max_bytes, int32_t max_rows, int32_t max_nnz, int32_t device_id,
                                ffm_textparse **out) {
  if (!out) return fail(FFM_E_INVALID, "null output");
  *out = nullptr;
  if (max_bytes < 1 || max_bytes > (static_cast<int64_t>(1) << 31) - 4096)
    return fail(FFM_E_INVALID, "max_bytes must lie in [1, 2^31 - 4096]: positions in a text are 32-bit");
  if (max_rows < 1 || max_nnz < 1 || max_rows == INT32_MAX) return fail(FFM_E_INVALID, "max_rows and max_nnz must be positive");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
    (void)hipGetLastError();
    return fail(FFM_E_DEVICE, "no HIP device: a text parser runs on the GPU (ffm_engine_textparse_host is the host twin)");
  }
  if (device_id < 0 || device_id >= n_dev) return fail(FFM_E_INVALID, "device_id out of range");
  HIP_TRY(hipSetDevice(device_id));
  ffm_textparse *p = new (std::nothrow) ffm_textparse;
  if (!p) return fail(FFM_E_NOMEM, "out of host memory");
  p->has_field = has_field ? 1 : 0;
  p->max_bytes = max_bytes;
  p->max_rows = max_rows;
  p->max_nnz = max_nnz;
  p->device_id = device_id;
  if (int rc = textparse_init(p)) {
    const std::string msg = g_last_error;
    ffm_engine_textparse_destroy(p);
    return fail(rc, msg);
  }
  *out = p;
  return FFM_OK;
}

// The slot's row_ptr [n_rows + 1] to its page-locked mirror, behind the parse on the parser's stream (rows_mirror_kernel,
// kernels_rows.h; the grid by the rows n_bytes of text can hold at two bytes a row, a real row being hundreds).
static void textparse_mirror(ffm_textparse *p, ffm_textparse::Slot &s, int64_t n_bytes) {
  const int grid = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(64, n_bytes / (64 * 256))));
  hipLaunchKernelGGL(rows_mirror_kernel, dim3(grid), dim3(256), 0, p->stream, s.d_row_ptr, s.d_counters, s.d_row_ptr_mirror,
                     static_cast<unsigned>(p->max_rows));
}

int ffm_engine_textparse_parse(ffm_textparse *p, int32_t slot, const char *text, int64_t n_bytes, int32_t zero_copy) {
  if (!p) return fail(FFM_E_INVALID, "null text parser");
  if (slot != 0 && slot != 1) return fail(FFM_E_INVALID, "slot must be 0 or 1");
  if (n_bytes < 0 || n_bytes > p->max_bytes) return fail(FFM_E_INVALID, "n_bytes must lie in [0, max_bytes]");
  if (n_bytes > 0 && !text) return fail(FFM_E_INVALID, "null text");
  ffm_textparse::Slot &s = p->slot[slot];
  if (s.in_flight) return fail(FFM_E_INVALID, "the slot's last parse was not waited for (ffm_engine_textparse_wait)");
  HIP_TRY(hipSetDevice(p->device_id));
  if (n_bytes > 0) {
    const char *src = text;
    if (zero_copy) {
      // the caller's page-locked text, copied by DMA; back at once, read until the slot's wait
      void *mapped = nullptr;
      if (hipHostGetDevicePointer(&mapped, const_cast<char *>(text), 0) != hipSuccess || !mapped) {
        (void)hipGetLastError();
        return fail(FFM_E_INVALID, "zero_copy text must be page-locked, device-mapped host memory (ffm_engine_pin_host)");
      }
    } else {
      if (!s.pinned) HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&s.pinned), static_cast<size_t>(p->max_bytes), hipHostMallocPortable));
      std::memcpy(s.pinned, text, static_cast<size_t>(n_bytes));
      src = s.pinned;
    }
    HIP_TRY(hipMemcpyAsync(s.d_text, src, static_cast<size_t>(n_bytes), hipMemcpyHostToDevice, p->stream));
  }
  TextArgs a{};
  a.text = s.d_text;
  a.n_bytes = static_cast<int32_t>(n_bytes);
  a.has_field = p->has_field;
  a.max_rows = p->max_rows;
  a.max_nnz = p->max_nnz;
  a.cap_lines = p->cap_lines;
  a.cap_btiles = p->cap_btiles;
  a.cap_ltiles = p->cap_ltiles;
  a.line_start = s.d_line_start;
  a.info = s.d_info;
  a.btile = s.d_btile;
  a.ltile_rows = s.d_ltile_rows;
  a.ltile_nnz = s.d_ltile_nnz;
  a.counters = s.d_counters;
  a.row_ptr = s.d_row_ptr;
  a.field = s.d_field;
  a.feat = s.d_feat;
  a.label = s.d_label;
  a.val = s.d_val;
  const int btiles = static_cast<int>((n_bytes + kTextScanBytes - 1) / kTextScanBytes);
  const int grid_b = std::max(1, std::min(2048, btiles));
  // (the number of lines is only known on the device: the line passes stride over the tiles from a grid sized by
  //  the most lines the bytes can hold, a line of a real file being tens of bytes at the least)
  const int grid_l = std::max(1, std::min(4096, static_cast<int>(n_bytes / (16 * kTextLineTile)) + 1));
  hipLaunchKernelGGL(text_count_newlines_kernel, dim3(grid_b), dim3(kTextThreads), 0, p->stream, a);
  hipLaunchKernelGGL((text_scan_kernel<0>), dim3(1), dim3(kTextScanChunk), 0, p->stream, a);
  hipLaunchKernelGGL(text_line_starts_kernel, dim3(grid_b), dim3(kTextThreads), 0, p->stream, a);
  hipLaunchKernelGGL((text_lines_kernel<false>), dim3(grid_l), dim3(kTextThreads), 0, p->stream, a);
  hipLaunchKernelGGL((text_scan_kernel<1>), dim3(1), dim3(kTextScanChunk), 0, p->stream, a);
  hipLaunchKernelGGL((text_lines_kernel<true>), dim3(grid_l), dim3(kTextThreads), 0, p->stream, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(s.h_counters, s.d_counters, sizeof(long long) * TC_COUNT, hipMemcpyDeviceToHost, p->stream));
  s.mirror_copied = false;
  s.mirror_rows = -1;
  if (p->mirror_on) {
    textparse_mirror(p, s, n_bytes);
    HIP_TRY(hipGetLastError());
    s.mirror_copied = true;
  }
  HIP_TRY(hipEventRecord(s.ev_done, p->stream));
  s.in_flight = true;
  return FFM_OK;
}

int ffm_engine_textparse_wait(ffm_textparse *p, int32_t slot, ffm_text_block *out) {
  if (!p) return fail(FFM_E_INVALID, "null text parser");
  if (slot != 0 && slot != 1) return fail(FFM_E_INVALID, "slot must be 0 or 1");
  if (!out) return fail(FFM_E_INVALID, "null output");
  ffm_textparse::Slot &s = p->slot[slot];
  if (!s.in_flight) return fail(FFM_E_INVALID, "nothing was parsed into this slot since its last wait");
  HIP_TRY(hipSetDevice(p->device_id));
  HIP_TRY(hipEventSynchronize(s.ev_done));
  s.in_flight = false;
  const long long *c = s.h_counters;
  out->n_lines = c[TC_LINES];
  out->n_rows = c[TC_ROWS];
  out->nnz = c[TC_NNZ];
  out->n_slow = c[TC_SLOW];
  out->first_slow_byte = c[TC_SLOW] ? c[TC_FIRST_SLOW] : -1;
  out->overflow = static_cast<int32_t>(c[TC_OVERFLOW]);
  out->row_ptr = s.d_row_ptr;
  out->field = s.d_field;
  out->feat = s.d_feat;
  out->label = s.d_label;
  out->val = s.d_val;
  return FFM_OK;
}

// _wait, and the page-locked host mirror of the slot's row_ptr [n_rows + 1] (include/ffm_engine.h "Resident rows"):
// what the host needs of a chunk to cut blocks out of it.  The first such wait makes the mirrors and copies its own
// slot's behind the parse; from then on every parse copies its slot's on the parser's stream, ahead of the slot's event.
int ffm_engine_textparse_wait_rows(ffm_textparse *p, int32_t slot, ffm_text_block *out, const int32_t **row_ptr_host) {
  if (!row_ptr_host) return fail(FFM_E_INVALID, "null output");
  *row_ptr_host = nullptr;
  if (int rc = ffm_engine_textparse_wait(p, slot, out)) return rc;
  ffm_textparse::Slot &s = p->slot[slot];
  if (out->n_slow != 0 || out->overflow != 0) return FFM_OK;  // (the arrays are not valid: nothing to mirror)
  if (!p->mirror_on) {
    for (auto &t : p->slot)
      if (!t.h_row_ptr) {
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&t.h_row_ptr), sizeof(int32_t) * (static_cast<size_t>(p->max_rows) + 1),
                              hipHostMallocPortable | hipHostMallocMapped));
        HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&t.d_row_ptr_mirror), t.h_row_ptr, 0));
      }
    p->mirror_on = true;
  }
  if (!s.mirror_copied) {
    textparse_mirror(p, s, static_cast<int64_t>(out->n_rows) * 2);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(p->stream));
    s.mirror_copied = true;
  }
  s.mirror_rows = out->n_rows;
  *row_ptr_host = s.h_row_ptr;
  return FFM_OK;
}

// The grammar on the host (no device needed): the device's bits (csrc/text_parse.h).
int ffm_engine_textparse_host(int32_t has_field, const char *text, int64_t n_bytes, int32_t max_rows, int32_t max_nnz, int32_t *row_ptr,
                              int32_t *field, int32_t *feat, float *val, int32_t *label, ffm_text_block *out) {
  if (!out) return fail(FFM_E_INVALID, "null output");
  if (n_bytes < 0 || n_bytes > (static_cast<int64_t>(1) << 31) - 4096) return fail(FFM_E_INVALID, "n_bytes must lie in [0, 2^31 - 4096]");
  if (n_bytes > 0 && !text) return fail(FFM_E_INVALID, "null text");
  if (max_rows < 0 || max_nnz < 0 || max_rows == INT32_MAX) return fail(FFM_E_INVALID, "negative capacity");
  if (!row_ptr || (max_rows > 0 && !label) || (max_nnz > 0 && (!field || !feat || !val))) return fail(FFM_E_INVALID, "null array");
  const ftrl_text::Totals t =
      ftrl_text::parse_block_host(has_field != 0, text, static_cast<int32_t>(n_bytes), max_rows, max_nnz, row_ptr, field, feat, val, label);
  out->n_lines = t.n_lines;
  out->n_rows = t.n_rows;
  out->nnz = t.nnz;
  out->n_slow = t.n_slow;
  out->first_slow_byte = t.first_slow_byte;
  out->overflow = t.overflow;
  out->row_ptr = out->field = out->feat = out->label = nullptr;
  out->val = nullptr;
  return FFM_OK;
}
