// engine_norm.h -- FFM_FLAG_NORM_ROWS: every row of a host block scaled to unit length on the device
// (kernels_norm.h; include/ffm_engine.h "Normalised rows").  The launch that stage_block and the staged uploads
// put behind the block's copy and id rewriting, ffm_engine_normalize_rows_device for callers of the _device entry
// points, the host twin and the counters.
// Part of engine.hip's translation unit (included inside its extern "C" block).

// The counter of rows left unscaled: made at create on a flagged engine, by the first
// ffm_engine_normalize_rows_device on any other.
static int norm_ready(ffm_engine *e) {
  if (e->d_norm_unscaled) return FFM_OK;
  if (int rc = e->alloc(&e->d_norm_unscaled, 1)) return rc;
  HIP_TRY(hipMemsetAsync(e->d_norm_unscaled, 0, sizeof(unsigned long long), e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return FFM_OK;
}

// What the kernel takes for a block in device memory (field: null on LR / FM and where the rows have none).
static NormJob norm_job(const ffm_engine *e, const Rows &rows, float *val_out) {
  const bool ffm = e->m.type == FFM_MODEL_FFM;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(ffm ? rows.field : nullptr) | reinterpret_cast<uintptr_t>(rows.feat) |
                         reinterpret_cast<uintptr_t>(rows.val) | reinterpret_cast<uintptr_t>(val_out);
  return NormJob{rows.n_rows, rows.nnz, rows.row_ptr, ffm ? rows.field : nullptr, rows.feat, rows.val, val_out,
                 e->m.n_feats, ffm ? e->m.n_fields : 0, (bits & 15u) == 0 ? 1 : 0, e->d_norm_unscaled};
}

// One launch on stream `st`; counts the block's rows.  (Timed like the main stream's kernels while profiling is
// on -- submissions then all come from the caller's thread.)
static void launch_normalize_rows(ffm_engine *e, hipStream_t st, const NormJob &job) {
  if (job.n_rows <= 0) return;
  e->norm_rows.fetch_add(job.n_rows, std::memory_order_relaxed);
  const int grid = std::max(1, std::min(e->grid_norm, cdiv(job.n_rows, kNormRows)));
  if (e->prof_on) LAUNCH_ON(e, st, K_NORM_ROWS, normalize_rows_kernel, grid, kNormThreads, 0, job);
  else hipLaunchKernelGGL(normalize_rows_kernel, dim3(grid), dim3(kNormThreads), 0, st, job);
}

// For callers of the _device entry points, which take arrays as they are: the definition applied to a block that
// is already in HBM (val_out == val_in: in place).  Any engine, flagged or not; asynchronous on the engine's stream.
int ffm_engine_normalize_rows_device(ffm_engine *e, int32_t n_rows, int32_t nnz, const int32_t *row_ptr, const int32_t *field,
                                     const int32_t *feat, const float *val_in, float *val_out) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  if (n_rows < 0 || nnz < 0) return fail(FFM_E_INVALID, "negative n_rows / nnz");
  if (!row_ptr) return fail(FFM_E_INVALID, "null row_ptr");
  if (nnz > 0 && (!feat || !val_out)) return fail(FFM_E_INVALID, "null feat / val_out array");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  if (int rc = norm_ready(e)) return rc;
  if (int rc_e = eval_launch_pending(e)) return rc_e;
  launch_normalize_rows(e, e->stream, norm_job(e, Rows{n_rows, nnz, row_ptr, field, feat, val_in, nullptr}, val_out));
  HIP_TRY(hipGetLastError());
  return FFM_OK;
}

// The same definition in plain C++ (no device needed): the kernel's bits.  Every operation below is one IEEE
// rounding: this file is compiled without contraction, and the host has no fused multiply-add to contract into.
int ffm_engine_normalize_rows_host(int32_t model_type, int32_t n_feats, int32_t n_fields, int32_t n_rows, const int32_t *row_ptr,
                                   const int32_t *field, const int32_t *feat, const float *val_in, float *val_out) {
  if (model_type < FFM_MODEL_LR || model_type > FFM_MODEL_FFM) return fail(FFM_E_INVALID, "invalid model_type, expect LR(0), FM(1) or FFM(2)");
  if (n_feats <= 0) return fail(FFM_E_INVALID, "n_feats must be positive");
  const bool ffm = model_type == FFM_MODEL_FFM;
  if (ffm && n_fields <= 0) return fail(FFM_E_INVALID, "n_fields must be positive for FFM");
  if (n_rows < 0) return fail(FFM_E_INVALID, "negative n_rows");
  if (!row_ptr) return fail(FFM_E_INVALID, "null row_ptr");
  if (row_ptr[0] != 0) return fail(FFM_E_INVALID, "row_ptr[0] must be 0");
  for (int32_t r = 0; r < n_rows; r++)
    if (row_ptr[r + 1] < row_ptr[r]) return fail(FFM_E_INVALID, "row_ptr must be non-decreasing");
  if (row_ptr[n_rows] > 0 && (!feat || !val_out)) return fail(FFM_E_INVALID, "null feat / val_out array");
  const int F = ffm && field ? n_fields : 0;
  for (int32_t r = 0; r < n_rows; r++) {
    float s = 0.0f;
    for (int32_t p = row_ptr[r]; p < row_ptr[r + 1]; p++) {
      if (!norm_keeps(feat[p], F ? field[p] : 0, n_feats, F)) continue;
      const float v = val_in ? val_in[p] : 1.0f;
      s = s + v * v;
    }
    const bool scales = norm_scales(s);
    const float scale = scales ? 1.0f / std::sqrt(s) : 1.0f;
    for (int32_t p = row_ptr[r]; p < row_ptr[r + 1]; p++) {
      const float v = val_in ? val_in[p] : 1.0f;
      val_out[p] = scales ? v * scale : v;  // (a row that is not scaled keeps its bits)
    }
  }
  return FFM_OK;
}

// Rows that went through the kernel since create or the last reset, and how many of them were left unscaled.
int ffm_engine_norm_stats(ffm_engine *e, int32_t reset, int64_t *rows, int64_t *unscaled) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  unsigned long long left = 0;
  if (e->d_norm_unscaled) {
    // every launch counted so far has ended: the deferred evaluation block's, the staging thread's, both streams'
    if (int rc_e = eval_launch_pending(e)) return rc_e;
    if (int rc_w = e->drain()) return rc_w;
    if (e->prep) HIP_TRY(hipStreamSynchronize(e->prep));
    HIP_TRY(hipMemcpyAsync(&left, e->d_norm_unscaled, sizeof left, hipMemcpyDeviceToHost, e->stream));
    if (reset) HIP_TRY(hipMemsetAsync(e->d_norm_unscaled, 0, sizeof left, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  if (rows) *rows = e->norm_rows.load(std::memory_order_relaxed);
  if (unscaled) *unscaled = static_cast<int64_t>(left);
  if (reset) e->norm_rows.store(0, std::memory_order_relaxed);
  return FFM_OK;
}
