// engine_serve.h -- serving engines (include/ffm_engine.h "Serving engines"): FFM_FLAG_SERVE_F32 / _F16 make
// an engine that stores the bias, lin_w and a packed table of w alone (kernels_serve.h) and answers every
// prediction entry point; this file holds what create checks, the predict dispatch, the transfers between
// the packed table and host arrays, ffm_engine_pack_weights and ffm_engine_model_bytes.
// Part of engine.hip's translation unit (included inside its extern "C" block).

static_assert(sizeof(ffm_pack_stats) == PK_COUNT * sizeof(int64_t), "the kernel and the ABI agree on the counters");

// The shapes the wave kernels serve (launch_row_waves, engine_step.h): FFM, a whole model on this device, a k
// with a lane shape (engine_select.h: 4, 8, 16, 32, 64), rows one wave stages.
static int serve_create_check(const ffm_engine_config *cfg) {
  if ((cfg->flags & FFM_FLAG_SERVE_F32) && (cfg->flags & FFM_FLAG_SERVE_F16))
    return fail(FFM_E_INVALID, "FFM_FLAG_SERVE_F32 and FFM_FLAG_SERVE_F16 exclude each other");
  if (cfg->max_row_nnz > kPredLdsCap)
    return fail(FFM_E_INVALID, "a serving engine takes rows of at most " + std::to_string(kPredLdsCap) +
                                   " entries (max_row_nnz): it has no kernel for longer ones");
  if (cfg->model_type != FFM_MODEL_FFM) return fail(FFM_E_UNSUPPORTED, "serving engines are FFM only (not LR / FM)");
  if (cfg->n_shards > 1) return fail(FFM_E_UNSUPPORTED, "a serving engine is one whole model on one device (n_shards == 1)");
  if (!row_wave_fn(SERVE_F32, cfg->n_factors))
    return fail(FFM_E_UNSUPPORTED, "serving engines support n_factors 4, 8, 16, 32 or 64");
  return FFM_OK;
}

// ---- one context against many candidates (include/ffm_engine.h "Scoring candidates") --------------------

static int cand_common_check(ffm_engine *e, int32_t n_req, int32_t n_cand) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  if (!serving(e))
    return fail(FFM_E_UNSUPPORTED, "score_candidates needs a serving engine (FFM_FLAG_SERVE_F32 / _F16): "
                                   "ffm_engine_pack_weights copies a training engine's weights into one");
  MASK_REFUSE(e, "score_candidates");
  if (e->norm_rows_on)
    return fail(FFM_E_INVALID, "score_candidates is not available on an engine with FFM_FLAG_NORM_ROWS: the shared context "
                               "terms would need a scale per candidate");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  if (int rc_e = eval_launch_pending(e)) return rc_e;
  if (n_req < 0 || n_cand < 0) return fail(FFM_E_INVALID, "negative n_req / n_cand");
  if (n_cand > e->max_rows) return fail(FFM_E_CAPACITY, "more candidates than max_batch_rows");
  return FFM_OK;
}

// Both launches, on arrays in device memory.  ctx_cap >= 1; row_cap: the longest concatenated row, if known.
static int cand_launch(ffm_engine *e, int32_t n_req, const int32_t *ctx_ptr, const int32_t *ctx_field, const int32_t *ctx_feat,
                       const float *ctx_val, const int32_t *cand_req_ptr, int32_t n_cand, const int32_t *cand_ptr,
                       const int32_t *cand_field, const int32_t *cand_feat, const float *cand_val, int32_t cand_nnz,
                       int ctx_cap, int row_cap, int32_t output_prob, float *out) {
  const size_t stride = static_cast<size_t>(cand_terms_stride(ctx_cap));
  int rc;
  if ((rc = e->grow(&e->cx.ent, &e->cx_ent_cap, static_cast<size_t>(n_req) * ctx_cap))) return rc;
  if ((rc = e->grow(&e->cx.head, &e->cx_head_cap, static_cast<size_t>(n_req)))) return rc;
  if ((rc = e->grow(&e->cx.terms, &e->cx_terms_cap, std::max<size_t>(1, static_cast<size_t>(n_req) * stride)))) return rc;
  if ((rc = e->grow(&e->cx.cand_req, &e->cx_cand_cap, static_cast<size_t>(n_cand)))) return rc;
  CandCtx cx = e->cx;
  cx.ctx_cap = ctx_cap;
  const ModelDev &m = e->m;
  const int ctx_lds = std::min(ctx_cap, kPredLdsCap), lds_cap = std::min(row_cap, kPredLdsCap);
  const size_t ctx_shmem = cand_ctx_lds_bytes(ctx_lds), shmem = pred_lds_bytes(lds_cap);
  const int ctx_grid = cdiv(n_req, kPredRows), grid = cdiv(n_cand, kPredRows), threads = 64 * kPredRows;
  const Rows rows{n_cand, cand_nnz, cand_ptr, cand_field, cand_feat, cand_val, nullptr};
  int *err = e->d_err;
  // (never null on a serving engine: create admitted only a k that has these kernels, serve_create_check)
  LAUNCH(e, K_SERVE_CTX, serve_context_fn(m.lat_fmt, m.n_factors), ctx_grid, threads, ctx_shmem, m, n_req, ctx_ptr, ctx_field,
         ctx_feat, ctx_val, cand_req_ptr, n_cand, cx, e->max_row_nnz, ctx_lds, err);
  LAUNCH(e, K_SERVE_CAND, serve_candidate_fn(m.lat_fmt, m.n_factors), grid, threads, shmem, m, n_req, ctx_ptr, cx, rows, row_cap,
         lds_cap, err, out, output_prob);
  HIP_TRY(hipGetLastError());
  return FFM_OK;
}

int ffm_engine_score_candidates_device(ffm_engine *e, int32_t n_req, const int32_t *ctx_ptr, const int32_t *ctx_field,
                                       const int32_t *ctx_feat, const float *ctx_val, const int32_t *cand_req_ptr,
                                       int32_t n_cand, const int32_t *cand_ptr, const int32_t *cand_field,
                                       const int32_t *cand_feat, const float *cand_val, int32_t ctx_nnz, int32_t cand_nnz,
                                       int32_t ctx_cap, int32_t output_prob, float *out) {
  if (int rc = cand_common_check(e, n_req, n_cand)) return rc;
  if (n_req == 0 || n_cand == 0) return FFM_OK;
  if (ctx_nnz < 0 || cand_nnz < 0 || ctx_cap < 0) return fail(FFM_E_INVALID, "negative ctx_nnz / cand_nnz / ctx_cap");
  if (!ctx_ptr || !cand_req_ptr || !cand_ptr || !out || (ctx_nnz > 0 && (!ctx_field || !ctx_feat || !ctx_val)) ||
      (cand_nnz > 0 && (!cand_field || !cand_feat || !cand_val)))
    return fail(FFM_E_INVALID, "null array");
  // (a context beyond the engine's row limit is flagged by its kernel whatever the cap says)
  const int cap = std::max(1, std::min(ctx_cap, e->max_row_nnz));
  return cand_launch(e, n_req, ctx_ptr, ctx_field, ctx_feat, ctx_val, cand_req_ptr, n_cand, cand_ptr, cand_field, cand_feat,
                     cand_val, cand_nnz, cap, e->max_row_nnz, output_prob, out);
}

static int cand_check_ptr(const int32_t *ptr, int32_t n, const char *name) {
  if (ptr[0] != 0) return fail(FFM_E_INVALID, std::string(name) + "[0] must be 0");
  for (int32_t r = 0; r < n; r++)
    if (ptr[r + 1] < ptr[r]) return fail(FFM_E_INVALID, std::string(name) + " must be non-decreasing");
  return FFM_OK;
}

int ffm_engine_score_candidates(ffm_engine *e, int32_t n_req, const int32_t *ctx_ptr, const int32_t *ctx_field,
                                const int32_t *ctx_feat, const float *ctx_val, const int32_t *cand_req_ptr, int32_t n_cand,
                                const int32_t *cand_ptr, const int32_t *cand_field, const int32_t *cand_feat,
                                const float *cand_val, int32_t output_prob, float *out) {
  int rc = cand_common_check(e, n_req, n_cand);
  if (rc) return rc;
  if (n_req == 0 || n_cand == 0) return FFM_OK;
  // ---- on the caller's thread, before anything is queued
  if (!ctx_ptr || !cand_req_ptr || !cand_ptr || !out) return fail(FFM_E_INVALID, "null array");
  if ((rc = cand_check_ptr(ctx_ptr, n_req, "ctx_ptr"))) return rc;
  if ((rc = cand_check_ptr(cand_req_ptr, n_req, "cand_req_ptr"))) return rc;
  if (cand_req_ptr[n_req] != n_cand) return fail(FFM_E_INVALID, "cand_req_ptr[n_req] must be n_cand");
  if ((rc = cand_check_ptr(cand_ptr, n_cand, "cand_ptr"))) return rc;
  const int32_t ctx_nnz = ctx_ptr[n_req], cand_nnz = cand_ptr[n_cand];
  if ((ctx_nnz > 0 && (!ctx_field || !ctx_feat)) || (cand_nnz > 0 && (!cand_field || !cand_feat)))
    return fail(FFM_E_INVALID, "null field / feat array");
  if (cand_nnz > e->max_nnz) return fail(FFM_E_CAPACITY, "the candidates exceed max_batch_nnz");
  int ctx_cap = 1, longest = 1;
  for (int32_t r = 0; r < n_req; r++) {
    const int nc = ctx_ptr[r + 1] - ctx_ptr[r];
    int most = 0;
    for (int32_t c = cand_req_ptr[r]; c < cand_req_ptr[r + 1]; c++) most = std::max(most, cand_ptr[c + 1] - cand_ptr[c]);
    if (nc + most > e->max_row_nnz)
      return fail(FFM_E_CAPACITY, "a context and candidate together have more entries than max_row_nnz");
    ctx_cap = std::max(ctx_cap, nc);
    longest = std::max(longest, nc + most);
  }
  const size_t n_ptr = static_cast<size_t>(n_req) + 1, n_ctx = std::max<size_t>(1, static_cast<size_t>(ctx_nnz));
  if ((rc = e->grow(&e->d_ctx_ptr, &e->ctx_ptr_cap, n_ptr))) return rc;
  if ((rc = e->grow(&e->d_req_ptr, &e->req_ptr_cap, n_ptr))) return rc;
  if ((rc = e->grow(&e->d_ctx_field, &e->ctx_field_cap, n_ctx))) return rc;
  if ((rc = e->grow(&e->d_ctx_feat, &e->ctx_feat_cap, n_ctx))) return rc;
  if ((rc = e->grow(&e->d_ctx_val, &e->ctx_val_cap, n_ctx))) return rc;
  // ---- copies, the values nobody sent, hashed ids: behind one another on the engine's stream, as stage_block
  hipStream_t st = e->stream;
  HIP_TRY(hipMemcpyAsync(e->d_ctx_ptr, ctx_ptr, sizeof(int32_t) * (n_req + 1), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(e->d_req_ptr, cand_req_ptr, sizeof(int32_t) * (n_req + 1), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(e->d_row_ptr, cand_ptr, sizeof(int32_t) * (n_cand + 1), hipMemcpyHostToDevice, st));
  struct Side { int32_t nnz; const int32_t *field, *feat; const float *val; int *d_field, *d_feat; float *d_val; };
  const Side sides[2] = {{ctx_nnz, ctx_field, ctx_feat, ctx_val, e->d_ctx_field, e->d_ctx_feat, e->d_ctx_val},
                         {cand_nnz, cand_field, cand_feat, cand_val, e->d_field, e->d_feat, e->d_val}};
  for (const Side &s : sides) {
    if (s.nnz <= 0) continue;
    HIP_TRY(hipMemcpyAsync(s.d_field, s.field, sizeof(int32_t) * s.nnz, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s.d_feat, s.feat, sizeof(int32_t) * s.nnz, hipMemcpyHostToDevice, st));
    if (s.val) HIP_TRY(hipMemcpyAsync(s.d_val, s.val, sizeof(float) * s.nnz, hipMemcpyHostToDevice, st));
    else
      hipLaunchKernelGGL(fill_ones_kernel, dim3(std::max(1, std::min(256, cdiv(cdiv(s.nnz, 4), 256)))), dim3(256), 0, st, s.d_val,
                         static_cast<unsigned>(s.nnz));
    if (e->hash_ids) launch_hash_ids(e, st, s.nnz, s.d_field, s.d_feat, s.d_feat, s.d_val);
  }
  rc = cand_launch(e, n_req, e->d_ctx_ptr, e->d_ctx_field, e->d_ctx_feat, e->d_ctx_val, e->d_req_ptr, n_cand, e->d_row_ptr,
                   e->d_field, e->d_feat, e->d_val, cand_nnz, ctx_cap, longest, output_prob, e->d_out);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(out, e->d_out, sizeof(float) * n_cand, hipMemcpyDeviceToHost, st));
  return check_device_errors(e);
}

// ---- packed table <-> host arrays (fp32 on the host; rounded / decoded on the device) ------------------

static int serve_vec_transfer(ffm_engine *e, float *host, bool to_host) {
  const int64_t RL = e->logical_len;
  const int64_t chunk = e->stage_floats / RL;
  for (int64_t f0 = 0; f0 < e->m.n_feats; f0 += chunk) {
    const int64_t nf = std::min<int64_t>(chunk, e->m.n_feats - f0);
    const size_t bytes = static_cast<size_t>(nf * RL) * sizeof(float);
    if (!to_host) HIP_TRY(hipMemcpyAsync(e->d_stage, host + f0 * RL, bytes, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(serve_dense_copy_kernel, dim3(1024), dim3(256), 0, e->stream, e->m, e->d_stage, f0, nf, to_host ? 1 : 0);
    if (to_host) HIP_TRY(hipMemcpyAsync(host + f0 * RL, e->d_stage, bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  return FFM_OK;
}

// One chunk of ffm_engine_get_rows / set_rows: the nf ids already in e->d_ids.
static int serve_rows_vec_transfer(ffm_engine *e, int nf, float *host, bool to_host) {
  const size_t bytes = static_cast<size_t>(nf) * e->logical_len * sizeof(float);
  if (!to_host) HIP_TRY(hipMemcpyAsync(e->d_stage, host, bytes, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(serve_rows_copy_kernel, dim3(1024), dim3(256), 0, e->stream, e->m, e->d_stage, e->d_ids,
                     static_cast<int64_t>(nf), to_host ? 1 : 0);
  if (to_host) HIP_TRY(hipMemcpyAsync(host, e->d_stage, bytes, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return FFM_OK;
}

// ---- a training engine's stored weights into a serving engine ------------------------------------------

int ffm_engine_pack_weights(ffm_engine *dst, ffm_engine *src, ffm_pack_stats *out) {
  if (out) std::memset(out, 0, sizeof(*out));
  if (!dst || !src) return fail(FFM_E_INVALID, "null engine");
  if (!serving(dst)) return fail(FFM_E_INVALID, "pack_weights: dst must be a serving engine (FFM_FLAG_SERVE_F32 / _F16)");
  if (serving(src)) return fail(FFM_E_INVALID, "pack_weights: src must be a training engine");
  if (src->m.type != FFM_MODEL_FFM || src->m.n_shards > 1)
    return fail(FFM_E_INVALID, "pack_weights: src must be a whole (unsharded) FFM model");
  if (src->m.n_feats != dst->m.n_feats || src->m.n_fields != dst->m.n_fields || src->m.n_factors != dst->m.n_factors)
    return fail(FFM_E_INVALID, "pack_weights: src and dst differ in (n_feats, n_fields, n_factors)");
  if (src->cfg.device_id != dst->cfg.device_id) return fail(FFM_E_INVALID, "pack_weights: src and dst live on different devices");
  if (src->has_pending) return fail(FFM_E_INVALID, "the previous block still awaits train_update");
  HIP_TRY(hipSetDevice(src->cfg.device_id));
  // src is drained as ffm_engine_refresh_weights drains it; dst's deferred evaluation block sees dst as it was
  if (int rc_e = eval_launch_pending(src)) return rc_e;
  while (src->n_staged > 0)
    if (int rc_t = train_one_staged(src)) return rc_t;
  if (int rc_d = check_device_errors(src)) return rc_d;
  if (int rc_e = eval_launch_pending(dst)) return rc_e;
  if (!dst->d_pack)
    if (int rc = dst->alloc(&dst->d_pack, static_cast<size_t>(PK_COUNT * kPackLine))) return rc;
  // src's stream is idle here (check_device_errors waits); the pass runs on dst's, behind what dst has queued
  int cus = 0;
  HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dst->cfg.device_id));
  const int64_t items = std::max<int64_t>(static_cast<int64_t>(src->m.n_feats) * (src->m.row_len / 4), src->m.n_feats);
  const int grid = static_cast<int>(std::min<int64_t>(std::max(1, cus) * 8, std::max<int64_t>(1, (items + kPackThreads - 1) / kPackThreads)));
  HIP_TRY(hipMemsetAsync(dst->d_pack, 0, PK_COUNT * kPackLine * sizeof(unsigned long long), dst->stream));
  const auto pack = dst->m.lat_fmt == SERVE_F16 ? serve_pack_kernel<SERVE_F16> : serve_pack_kernel<SERVE_F32>;
  hipLaunchKernelGGL(pack, dim3(grid), dim3(kPackThreads), 0, dst->stream, src->m, dst->m, dst->d_pack);
  HIP_TRY(hipGetLastError());
  unsigned long long h[PK_COUNT * kPackLine] = {};
  HIP_TRY(hipMemcpyAsync(h, dst->d_pack, sizeof(h), hipMemcpyDeviceToHost, dst->stream));
  HIP_TRY(hipStreamSynchronize(dst->stream));
  if (out) {
    out->n_latent = static_cast<int64_t>(h[PK_LATENT * kPackLine]);
    out->n_inexact = static_cast<int64_t>(h[PK_INEXACT * kPackLine]);
    out->n_to_inf = static_cast<int64_t>(h[PK_TO_INF * kPackLine]);
    out->n_to_zero = static_cast<int64_t>(h[PK_TO_ZERO * kPackLine]);
  }
  return FFM_OK;
}

// Bytes of HBM requested for the model arrays: bias, linear, latent.
int64_t ffm_engine_model_bytes(const ffm_engine *e) {
  if (!e) return 0;
  const int64_t nf = e->m.n_feats, n_w = e->n_records * static_cast<int64_t>(e->m.row_len);
  if (serving(e)) return 4 + 4 * nf + (e->m.lat_fmt == SERVE_F16 ? 2 : 4) * n_w;
  return 12 + 12 * nf + 12 * n_w;
}
