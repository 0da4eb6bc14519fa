// engine_serve.h -- serving engines (include/ffm_engine.h "Serving engines"): FFM_FLAG_SERVE_F32 / _F16 make
// an engine that stores the bias, lin_w and a packed table of w alone (kernels_serve.h) and answers every
// prediction entry point; this file holds what create checks, the predict dispatch, the transfers between
// the packed table and host arrays, ffm_engine_pack_weights and ffm_engine_model_bytes.
// Part of engine.hip's translation unit (included inside its extern "C" block).

static_assert(sizeof(ffm_pack_stats) == PK_COUNT * sizeof(int64_t), "the kernel and the ABI agree on the counters");

// The shapes launch_predict_waves serves: FFM, a whole model on this device, k in {4, 8, 16, 32, 64}, rows
// one wave stages.
static int serve_create_check(const ffm_engine_config *cfg) {
  if ((cfg->flags & FFM_FLAG_SERVE_F32) && (cfg->flags & FFM_FLAG_SERVE_F16))
    return fail(FFM_E_INVALID, "FFM_FLAG_SERVE_F32 and FFM_FLAG_SERVE_F16 exclude each other");
  if (cfg->max_row_nnz > kPredLdsCap)
    return fail(FFM_E_INVALID, "a serving engine takes rows of at most " + std::to_string(kPredLdsCap) +
                                   " entries (max_row_nnz): it has no kernel for longer ones");
  if (cfg->model_type != FFM_MODEL_FFM) return fail(FFM_E_UNSUPPORTED, "serving engines are FFM only (not LR / FM)");
  if (cfg->n_shards > 1) return fail(FFM_E_UNSUPPORTED, "a serving engine is one whole model on one device (n_shards == 1)");
  const int k = cfg->n_factors;
  if (k != 4 && k != 8 && k != 16 && k != 32 && k != 64)
    return fail(FFM_E_UNSUPPORTED, "serving engines support n_factors 4, 8, 16, 32 or 64");
  return FFM_OK;
}

static void launch_serve_waves(ffm_engine *e, const Rows &rows, int row_cap, float *out, int output_prob) {
  const ModelDev &m = e->m;
  const int lds_cap = std::min(row_cap, kPredLdsCap);
  const size_t shmem = pred_lds_bytes(lds_cap);
  const int grid = cdiv(rows.n_rows, kPredRows), threads = 64 * kPredRows;
  // (the lane shapes of launch_predict_waves, engine_step.h)
#define SERVE_LAUNCH(LPP, VPL, U)                                                                                          \
  do {                                                                                                                      \
    if (m.lat_fmt == SERVE_F16)                                                                                             \
      LAUNCH(e, K_SERVE_ROW, (ffm_serve_wave_kernel<SERVE_F16, LPP, VPL, U>), grid, threads, shmem, m, rows, e->sc[e->cur], \
             row_cap, lds_cap, out, output_prob);                                                                           \
    else                                                                                                                    \
      LAUNCH(e, K_SERVE_ROW, (ffm_serve_wave_kernel<SERVE_F32, LPP, VPL, U>), grid, threads, shmem, m, rows, e->sc[e->cur], \
             row_cap, lds_cap, out, output_prob);                                                                           \
  } while (0)
  switch (m.n_factors) {
    case 4: SERVE_LAUNCH(1, 1, 4); break;
    case 8: SERVE_LAUNCH(2, 1, 4); break;
    case 16: SERVE_LAUNCH(FFM_PRED_LPP, 4 / FFM_PRED_LPP, FFM_PRED_U); break;
    case 32: SERVE_LAUNCH(8, 1, 2); break;
    default: SERVE_LAUNCH(16, 1, 1); break;  // 64 (create admits nothing else)
  }
#undef SERVE_LAUNCH
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
  if (dst->m.lat_fmt == SERVE_F16)
    hipLaunchKernelGGL(serve_pack_kernel<SERVE_F16>, dim3(grid), dim3(kPackThreads), 0, dst->stream, src->m, dst->m, dst->d_pack);
  else
    hipLaunchKernelGGL(serve_pack_kernel<SERVE_F32>, dim3(grid), dim3(kPackThreads), 0, dst->stream, src->m, dst->m, dst->d_pack);
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
