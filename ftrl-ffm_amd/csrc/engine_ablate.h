// engine_ablate.h -- field ablation (include/ffm_engine.h "Field ablation"): ffm_engine_ablation_enable makes
// the variant-major scratch, ffm_engine_predict_ablated[_device] run ffm_ablate_wave_kernel (kernels_ablate.h)
// and, per variant, the loss sum and the score histogram; ffm_engine_ablation_read reduces the histograms on the
// host as ffm_engine_metrics_read does.  Nothing here feeds the metric channels or the keyed capture, and an
// engine that never calls ffm_engine_ablation_enable allocates and launches nothing of it.
// (The kernel's dynamic LDS is pred_lds_bytes(kPredLdsCap) = 12 KB at the most, like the other wave kernels':
// within the default limit, so opt_in_lds has nothing to ask for.)
// Part of engine.hip's translation unit (included inside its extern "C" block).

static int ablate_variants(const ffm_engine *e) { return e->m.n_fields + 1; }

int ffm_engine_ablation_enable(ffm_engine *e, int32_t with_auc) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  const ModelDev &m = e->m;
  if (m.type != FFM_MODEL_FFM) return fail(FFM_E_UNSUPPORTED, "field ablation is FFM only: LR and FM rows have no fields");
  if (m.n_shards > 1 || e->in_group)
    return fail(FFM_E_UNSUPPORTED, "field ablation needs a whole model on one device (n_shards == 1, not a group's engine)");
  if (m.field_start || m.own_n || m.lin_own)
    return fail(FFM_E_UNSUPPORTED, "field ablation needs full-length records (not a shard's compact storage)");
  if (!ablate_wave_fn(m.lat_fmt, m.n_factors))
    return fail(FFM_E_UNSUPPORTED, "field ablation supports n_factors 4, 8, 16, 32 or 64 (the wave kernels' lane shapes)");
  if (m.n_fields > 64)
    return fail(FFM_E_UNSUPPORTED, "field ablation supports at most 64 fields: a row is one wave and a variant one lane of it");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  if (int rc_e = eval_launch_pending(e)) return rc_e;
  const size_t V = static_cast<size_t>(ablate_variants(e)), R = static_cast<size_t>(std::max(1, e->max_rows));
  int rc;
  if (!e->abl.out) {
    if ((rc = e->alloc(&e->abl.out, V * R)) || (rc = e->alloc(&e->abl.loss, V * R)) || (rc = e->alloc(&e->abl.sums, V)) ||
        (rc = e->alloc(&e->abl.part, V * (kLossParts + 1))))
      return rc;
    HIP_TRY(hipMemsetAsync(e->abl.part, 0, sizeof(double) * V * (kLossParts + 1), e->stream));
  }
  if (with_auc && !e->abl.auc) {  // (a channel that turns on starts from zero, one that stays on keeps its counts)
    if (!e->abl.hist && (rc = e->alloc(&e->abl.hist, V * kMetricWords))) return rc;
    HIP_TRY(hipMemsetAsync(e->abl.hist, 0, sizeof(unsigned long long) * V * kMetricWords, e->stream));
  }
  e->abl.auc = with_auc != 0;
  e->abl.on = true;
  return FFM_OK;
}

// The launches, on a block in device memory; row_cap as launch_row_kernel takes it.  out / loss_sum_out: device
// arrays of the variants' scores and loss sums, or null (the scores then stay in the engine's scratch).
static int ablate_core(ffm_engine *e, const Rows &rows, int row_cap, int32_t output_prob, float *out, double *loss_sum_out) {
  const ModelDev &m = e->m;
  const int V = ablate_variants(e), n_rows = rows.n_rows;
  float *const score = out ? out : e->abl.out;
  if (n_rows > 0) {
    if (row_cap <= 0) row_cap = e->max_row_nnz;
    const int lds_cap = std::min(row_cap, kPredLdsCap);
    hipLaunchKernelGGL(ablate_wave_fn(m.lat_fmt, m.n_factors), dim3(cdiv(n_rows, kPredRows)), dim3(64 * kPredRows),
                       pred_lds_bytes(lds_cap), e->stream, m, rows, e->d_err, row_cap, lds_cap, score, e->abl.loss, e->max_rows,
                       output_prob);
    if (rows.label && e->abl.auc)
      hipLaunchKernelGGL(ablate_hist_kernel, dim3(cdiv(n_rows, kMetricThreads), V), dim3(kMetricThreads), 0, e->stream, n_rows,
                         score, output_prob, rows.label, e->abl.hist);
  }
  if (loss_sum_out) {
    if (rows.label && n_rows > 0)
      hipLaunchKernelGGL(ablate_loss_sum_kernel, dim3(loss_grid(n_rows), V), dim3(256), 0, e->stream, n_rows, e->abl.loss,
                         e->max_rows, loss_sum_out, e->abl.part);
    else
      HIP_TRY(hipMemsetAsync(loss_sum_out, 0, sizeof(double) * V, e->stream));
  }
  HIP_TRY(hipGetLastError());
  return FFM_OK;
}

static int ablate_ready(ffm_engine *e) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  if (!e->abl.on) return fail(FFM_E_INVALID, "field ablation is off (ffm_engine_ablation_enable)");
  return FFM_OK;
}

int ffm_engine_predict_ablated_device(ffm_engine *e, int32_t n_rows, int32_t nnz, const int32_t *row_ptr, const int32_t *field,
                                      const int32_t *feat, const float *val, const int32_t *label, int32_t output_prob,
                                      float *out, double *loss_sum_out) {
  int rc = ablate_ready(e);
  if (rc) return rc;
  if ((rc = check_block(e, n_rows, nnz, row_ptr, field, feat, val))) return rc;
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  return ablate_core(e, Rows{n_rows, nnz, row_ptr, field, feat, val, label}, 0, output_prob, out, loss_sum_out);
}

int ffm_engine_predict_ablated(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr, const int32_t *field,
                               const int32_t *feat, const float *val, const int32_t *label, int32_t output_prob, float *out,
                               double *loss_sum_out) {
  int rc = ablate_ready(e);
  if (rc) return rc;
  Rows dev{};
  int row_cap = 0;
  if ((rc = stage_block(e, n_rows, row_ptr, field, feat, val, label, &dev, &row_cap))) return rc;
  const int V = ablate_variants(e);
  if ((rc = ablate_core(e, dev, row_cap, output_prob, nullptr, label ? e->abl.sums : nullptr))) return rc;
  if (out && n_rows > 0)
    HIP_TRY(hipMemcpyAsync(out, e->abl.out, sizeof(float) * V * n_rows, hipMemcpyDeviceToHost, e->stream));
  if (loss_sum_out) {
    if (label && n_rows > 0) HIP_TRY(hipMemcpyAsync(loss_sum_out, e->abl.sums, sizeof(double) * V, hipMemcpyDeviceToHost, e->stream));
    else std::fill(loss_sum_out, loss_sum_out + V, 0.0);
  }
  return check_device_errors(e);
}

int ffm_engine_ablation_read(ffm_engine *e, int32_t reset, ffm_metrics *out) {
  int rc = ablate_ready(e);
  if (rc) return rc;
  if (!out) return fail(FFM_E_INVALID, "null output");
  if (!e->abl.auc) return fail(FFM_E_INVALID, "field ablation was enabled without histograms (with_auc == 0)");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  if (int rc_e = eval_launch_pending(e)) return rc_e;
  const int V = ablate_variants(e);
  const size_t bytes = kMetricWords * sizeof(unsigned long long);
  std::vector<unsigned long long> h;
  try { h.assign(kMetricWords, 0ull); } catch (const std::bad_alloc &) { return fail(FFM_E_NOMEM, "host allocation failed"); }
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the counters are 64-bit");
  for (int v = 0; v < V; v++) {  // (one histogram at a time: 16 MiB of host memory, not 16 MiB per field)
    unsigned long long *const hist = e->abl.hist + static_cast<size_t>(v) * kMetricWords;
    HIP_TRY(hipMemcpyAsync(h.data(), hist, bytes, hipMemcpyDeviceToHost, e->stream));
    if (reset) HIP_TRY(hipMemsetAsync(hist, 0, bytes, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const uint64_t *w = reinterpret_cast<const uint64_t *>(h.data());
    if ((rc = ffm_engine_metrics_from_histogram(w, w + kMetricBins, kMetricBins,
                                                static_cast<int64_t>(w[2 * static_cast<size_t>(kMetricBins)]), out + v)))
      return rc;
  }
  return FFM_OK;
}
