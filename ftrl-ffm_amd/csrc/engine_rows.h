// engine_rows.h -- resident rows (include/ffm_engine.h "Resident rows"), host side: a row cutter -- a ring of block
// buffers in HBM, the launches of rows_take_kernel (kernels_rows.h) that fill them from a text parser's slots, the
// copies that fill them from rows the host parsed -- and the three staged entry points' twins for a block that is
// already in HBM (they share every step behind the source with the host forms: engine_stage.h).
// A cutter touches nothing of an engine.  Part of engine.hip's translation unit (inside its extern "C" block).

struct ffm_rowcut {
  int32_t max_rows = 0, max_nnz = 0, n_blocks = 0, device_id = 0;
  struct Buf {
    int32_t *row_ptr = nullptr, *field = nullptr, *feat = nullptr, *label = nullptr;
    float *val = nullptr;
    hipEvent_t ev_ready = nullptr;
    bool held = false;  // closed and not released: the engine may still read it
  };
  std::vector<Buf> ring;
  int cur = 0;                  // the buffer being assembled
  int32_t n_rows = 0, nnz = 0, longest = 0;  // ... and what it holds so far
  bool started = false;         // something was launched into it
  hipStream_t own = nullptr;    // take_host's copies, and the event of a block nothing was taken into
  hipStream_t last = nullptr;   // the stream of the block's last take (a parser's, or own)
  hipEvent_t ev_switch = nullptr;
  std::vector<int32_t> host_row_ptr;  // take_host's rebased row_ptr
};

void ffm_engine_rowcut_destroy(ffm_rowcut *c) {
  if (!c) return;
  (void)hipSetDevice(c->device_id);
  (void)hipDeviceSynchronize();  // (takes run on parsers' streams)
  for (auto &b : c->ring) {
    void *dev[] = {b.row_ptr, b.field, b.feat, b.label, b.val};
    for (void *d : dev)
      if (d) (void)hipFree(d);
    if (b.ev_ready) (void)hipEventDestroy(b.ev_ready);
  }
  if (c->ev_switch) (void)hipEventDestroy(c->ev_switch);
  if (c->own) (void)hipStreamDestroy(c->own);
  delete c;
}

static int rowcut_init(ffm_rowcut *c) {
  HIP_TRY(hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&c->ev_switch, hipEventDisableTiming));
  const size_t R = static_cast<size_t>(c->max_rows), E = static_cast<size_t>(c->max_nnz);
  c->ring.resize(static_cast<size_t>(c->n_blocks));
  for (auto &b : c->ring) {  // (hipMalloc aligns to far more than 16 bytes)
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&b.row_ptr), sizeof(int32_t) * (R + 1)));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&b.label), sizeof(int32_t) * R));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&b.field), sizeof(int32_t) * E));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&b.feat), sizeof(int32_t) * E));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&b.val), sizeof(float) * E));
    HIP_TRY(hipEventCreateWithFlags(&b.ev_ready, hipEventDisableTiming));
  }
  return FFM_OK;
}

int ffm_engine_rowcut_create(int32_t max_rows, int32_t max_nnz, int32_t n_blocks, int32_t device_id, ffm_rowcut **out) {
  if (!out) return fail(FFM_E_INVALID, "null output");
  *out = nullptr;
  if (max_rows < 1 || max_nnz < 1 || max_rows == INT32_MAX) return fail(FFM_E_INVALID, "max_rows and max_nnz must be positive");
  if (n_blocks < 1 || n_blocks > 64) return fail(FFM_E_INVALID, "n_blocks must lie in [1, 64]");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
    (void)hipGetLastError();
    return fail(FFM_E_DEVICE, "no HIP device: a row cutter's blocks lie in HBM");
  }
  if (device_id < 0 || device_id >= n_dev) return fail(FFM_E_INVALID, "device_id out of range");
  HIP_TRY(hipSetDevice(device_id));
  ffm_rowcut *c = new (std::nothrow) ffm_rowcut;
  if (!c) return fail(FFM_E_NOMEM, "out of host memory");
  c->max_rows = max_rows;
  c->max_nnz = max_nnz;
  c->n_blocks = n_blocks;
  c->device_id = device_id;
  if (int rc = rowcut_init(c)) {
    const std::string msg = g_last_error;
    ffm_engine_rowcut_destroy(c);
    return fail(rc, msg);
  }
  *out = c;
  return FFM_OK;
}

// What every take checks before anything is launched: the buffer is free, and the rows fit.
static int rowcut_room(ffm_rowcut *c, int64_t n_rows, int64_t n_entries) {
  if (c->ring[static_cast<size_t>(c->cur)].held)
    return fail(FFM_E_CAPACITY, "every block buffer of the cutter is held: release one (ffm_engine_rowcut_release) once its block was pulled");
  if (c->n_rows + n_rows > c->max_rows || c->nnz + n_entries > c->max_nnz)
    return fail(FFM_E_CAPACITY, "the rows do not fit into the cutter's block (max_rows / max_nnz)");
  return FFM_OK;
}

// The block's next launches go to `st`: behind everything the block's earlier ones put on another stream.
static int rowcut_on_stream(ffm_rowcut *c, hipStream_t st) {
  if (c->started && c->last != st) {
    HIP_TRY(hipEventRecord(c->ev_switch, c->last));
    HIP_TRY(hipStreamWaitEvent(st, c->ev_switch, 0));
  }
  c->last = st;
  c->started = true;
  return FFM_OK;
}

int ffm_engine_rowcut_take(ffm_rowcut *c, ffm_textparse *p, int32_t slot, int32_t r0, int32_t r1) {
  if (!c) return fail(FFM_E_INVALID, "null row cutter");
  if (!p) return fail(FFM_E_INVALID, "null text parser");
  if (slot != 0 && slot != 1) return fail(FFM_E_INVALID, "slot must be 0 or 1");
  if (p->device_id != c->device_id) return fail(FFM_E_INVALID, "the parser and the cutter lie on different devices");
  ffm_textparse::Slot &s = p->slot[slot];
  if (s.in_flight || s.mirror_rows < 0)
    return fail(FFM_E_INVALID, "the slot holds no block whose rows were mirrored (ffm_engine_textparse_wait_rows)");
  if (r0 < 0 || r1 < r0 || r1 > s.mirror_rows) return fail(FFM_E_INVALID, "rows [r0, r1) must lie inside the slot's block");
  const int32_t *rp = s.h_row_ptr;
  const int64_t e0 = rp[r0], e1 = rp[r1];
  int32_t longest = 0;
  for (int32_t r = r0; r < r1; r++) {
    if (rp[r + 1] < rp[r]) return fail(FFM_E_INVALID, "the slot's row_ptr is not non-decreasing");
    longest = std::max(longest, rp[r + 1] - rp[r]);
  }
  if (e0 < 0 || e1 < e0 || e1 > p->max_nnz) return fail(FFM_E_INVALID, "the slot's row_ptr leaves the slot's arrays");
  if (int rc = rowcut_room(c, r1 - r0, e1 - e0)) return rc;
  if (r1 == r0) return FFM_OK;
  HIP_TRY(hipSetDevice(c->device_id));
  if (int rc = rowcut_on_stream(c, p->stream)) return rc;
  ffm_rowcut::Buf &b = c->ring[static_cast<size_t>(c->cur)];
  RowTakeJob job{};
  job.src_row_ptr = s.d_row_ptr;
  job.src_field = s.d_field;
  job.src_feat = s.d_feat;
  job.src_label = s.d_label;
  job.src_val = s.d_val;
  job.dst_row_ptr = b.row_ptr;
  job.dst_field = b.field;
  job.dst_feat = b.feat;
  job.dst_label = b.label;
  job.dst_val = b.val;
  job.r0 = static_cast<unsigned>(r0);
  job.n_rows = static_cast<unsigned>(r1 - r0);
  job.e0 = static_cast<unsigned>(e0);
  job.n_entries = static_cast<unsigned>(e1 - e0);
  job.dst_row = static_cast<unsigned>(c->n_rows);
  job.dst_entry = static_cast<unsigned>(c->nnz);
  job.cap_rows = static_cast<unsigned>(c->max_rows);
  job.cap_entries = static_cast<unsigned>(c->max_nnz);
  // a lane moves four words of each array per step
  const int64_t vecs = std::max<int64_t>(e1 - e0, r1 - r0) / 4 + 1;
  const int grid = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(1024, (vecs + 255) / 256)));
  hipLaunchKernelGGL(rows_take_kernel, dim3(grid), dim3(256), 0, p->stream, job);
  HIP_TRY(hipGetLastError());
  c->n_rows += r1 - r0;
  c->nnz += static_cast<int32_t>(e1 - e0);
  c->longest = std::max(c->longest, longest);
  return FFM_OK;
}

// Rows the HOST parsed (a chunk the device will not parse): row_ptr [n_rows + 1] may start anywhere -- field / feat /
// val point at entry row_ptr[0], label at the first row --, so a part of a larger block is taken without a copy.
// The arrays are free when the call returns.
int ffm_engine_rowcut_take_host(ffm_rowcut *c, int32_t n_rows, const int32_t *row_ptr, const int32_t *field, const int32_t *feat,
                                const float *val, const int32_t *label) {
  if (!c) return fail(FFM_E_INVALID, "null row cutter");
  if (n_rows < 0) return fail(FFM_E_INVALID, "negative n_rows");
  if (!row_ptr) return fail(FFM_E_INVALID, "null row_ptr");
  int32_t longest = 0;
  for (int32_t r = 0; r < n_rows; r++) {
    if (row_ptr[r + 1] < row_ptr[r]) return fail(FFM_E_INVALID, "row_ptr must be non-decreasing");
    longest = std::max(longest, row_ptr[r + 1] - row_ptr[r]);
  }
  const int64_t n_entries = static_cast<int64_t>(row_ptr[n_rows]) - row_ptr[0];
  if ((n_rows > 0 && !label) || (n_entries > 0 && (!field || !feat || !val))) return fail(FFM_E_INVALID, "null CSR array");
  if (int rc = rowcut_room(c, n_rows, n_entries)) return rc;
  if (n_rows == 0) return FFM_OK;
  HIP_TRY(hipSetDevice(c->device_id));
  if (int rc = rowcut_on_stream(c, c->own)) return rc;
  ffm_rowcut::Buf &b = c->ring[static_cast<size_t>(c->cur)];
  // row_ptr rebased on the host; element 0 of the block's too where these are its first rows
  const bool first = c->n_rows == 0;
  c->host_row_ptr.resize(static_cast<size_t>(n_rows) + 1);
  for (int32_t r = 0; r <= n_rows; r++) c->host_row_ptr[static_cast<size_t>(r)] = row_ptr[r] - row_ptr[0] + c->nnz;
  const size_t skip = first ? 0 : 1;
  HIP_TRY(hipMemcpyAsync(b.row_ptr + c->n_rows + skip, c->host_row_ptr.data() + skip, sizeof(int32_t) * (static_cast<size_t>(n_rows) + 1 - skip),
                         hipMemcpyHostToDevice, c->own));
  HIP_TRY(hipMemcpyAsync(b.label + c->n_rows, label, sizeof(int32_t) * static_cast<size_t>(n_rows), hipMemcpyHostToDevice, c->own));
  if (n_entries > 0) {
    const size_t bytes = 4 * static_cast<size_t>(n_entries);
    HIP_TRY(hipMemcpyAsync(b.field + c->nnz, field, bytes, hipMemcpyHostToDevice, c->own));
    HIP_TRY(hipMemcpyAsync(b.feat + c->nnz, feat, bytes, hipMemcpyHostToDevice, c->own));
    HIP_TRY(hipMemcpyAsync(b.val + c->nnz, val, bytes, hipMemcpyHostToDevice, c->own));
  }
  HIP_TRY(hipStreamSynchronize(c->own));  // (the caller's arrays and host_row_ptr are free; the slow path may wait)
  c->n_rows += n_rows;
  c->nnz += static_cast<int32_t>(n_entries);
  c->longest = std::max(c->longest, longest);
  return FFM_OK;
}

int ffm_engine_rowcut_close(ffm_rowcut *c, ffm_rows_block *out) {
  if (!c) return fail(FFM_E_INVALID, "null row cutter");
  if (!out) return fail(FFM_E_INVALID, "null output");
  ffm_rowcut::Buf &b = c->ring[static_cast<size_t>(c->cur)];
  if (int rc = rowcut_room(c, 0, 0)) return rc;
  HIP_TRY(hipSetDevice(c->device_id));
  if (!c->started) {  // (a block of no rows: row_ptr[0] and nothing else)
    if (int rc = rowcut_on_stream(c, c->own)) return rc;
    HIP_TRY(hipMemsetAsync(b.row_ptr, 0, sizeof(int32_t), c->own));
  }
  HIP_TRY(hipEventRecord(b.ev_ready, c->last));
  out->n_rows = c->n_rows;
  out->nnz = c->nnz;
  out->longest_row = c->longest;
  out->index = c->cur;
  out->seq = 0;
  out->row_ptr = b.row_ptr;
  out->field = b.field;
  out->feat = b.feat;
  out->label = b.label;
  out->val = b.val;
  out->ready = b.ev_ready;
  b.held = true;
  c->cur = (c->cur + 1) % c->n_blocks;
  c->n_rows = c->nnz = c->longest = 0;
  c->started = false;
  c->last = nullptr;
  return FFM_OK;
}

int ffm_engine_rowcut_release(ffm_rowcut *c, int32_t index) {
  if (!c) return fail(FFM_E_INVALID, "null row cutter");
  if (index < 0 || index >= c->n_blocks) return fail(FFM_E_INVALID, "no such block buffer");
  if (!c->ring[static_cast<size_t>(index)].held) return fail(FFM_E_INVALID, "the block buffer is not held");
  c->ring[static_cast<size_t>(index)].held = false;
  return FFM_OK;
}

// ---- an engine stages a block that is already in HBM -------------------------------------------------------------

// What validate_host_block derives from a host row_ptr comes in with the block; the refusals are the host forms'.
static int validate_resident_block(ffm_engine *e, const ffm_rows_block *blk, Rows *dev, bool hold_eval) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  if (!blk) return fail(FFM_E_INVALID, "null block");
  const int32_t *field = e->m.type == FFM_MODEL_FFM ? blk->field : nullptr;
  if (blk->n_rows < 0) return fail(FFM_E_INVALID, "negative n_rows");
  if (!blk->row_ptr) return fail(FFM_E_INVALID, "null row_ptr");
  if (blk->n_rows > e->max_rows) return fail(FFM_E_CAPACITY, "block exceeds max_batch_rows");
  int rc = check_block(e, blk->n_rows, blk->nnz, blk->row_ptr, field, blk->feat, blk->val, false, false, hold_eval);
  if (rc) return rc;
  if (blk->longest_row < 0 || blk->longest_row > blk->nnz) return fail(FFM_E_INVALID, "longest_row must lie in [0, nnz]");
  if (blk->longest_row > e->max_row_nnz) return fail(FFM_E_CAPACITY, "a row has more entries than max_row_nnz");
  const void *arrays[] = {blk->row_ptr, field, blk->feat, blk->val, blk->label};
  for (const void *a : arrays)
    if (reinterpret_cast<uintptr_t>(a) & 15u) return fail(FFM_E_INVALID, "a resident block's arrays must be 16-byte aligned");
  *dev = Rows{blk->n_rows, blk->nnz, blk->row_ptr, field, blk->feat, blk->val, blk->label};
  return FFM_OK;
}

int ffm_engine_stage_batch_resident(ffm_engine *e, ffm_rows_block *blk) {
  SERVE_REFUSE(e, "training");
  MASK_REFUSE(e, "training");
  Rows dev{};
  int rc = validate_resident_block(e, blk, &dev, false);
  if (rc) return rc;
  if (blk->n_rows > 0 && !blk->label) return fail(FFM_E_INVALID, "training needs labels");
  if ((rc = stage_block_from(e, dev, std::max(1, blk->longest_row), nullptr, 1, true, static_cast<hipEvent_t>(blk->ready)))) return rc;
  blk->seq = e->n_staged_total;
  return FFM_OK;
}

int ffm_engine_train_batch_async_resident(ffm_engine *e, ffm_rows_block *blk) {
  if (e && e->m.n_shards > 1)
    return fail(FFM_E_INVALID, "sharded engines train with stage_batch + train_forward_staged + all-reduce + train_update");
  int rc = ffm_engine_stage_batch_resident(e, blk);
  if (rc) return rc;
  while (e->n_staged > 2)  // (the page-locked form's schedule: block t + 2 is staged, block t trains)
    if ((rc = train_one_staged(e))) return rc;
  return FFM_OK;
}

int ffm_engine_predict_batch_async_resident(ffm_engine *e, ffm_rows_block *blk, int32_t output_prob, float *scores_host) {
  Rows dev{};
  int rc = validate_resident_block(e, blk, &dev, true);
  if (rc) return rc;
  if ((rc = predict_block_from(e, dev, std::max(1, blk->longest_row), 1, true, static_cast<hipEvent_t>(blk->ready), output_prob, scores_host)))
    return rc;
  blk->seq = e->n_staged_total;
  return FFM_OK;
}
