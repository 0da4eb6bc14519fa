// engine_ablate_pairs.h -- pair ablation (include/ffm_engine.h "Pair ablation"): the numbering of the variants
// (host arithmetic, no device), ffm_engine_pair_ablation_enable makes the variant-major scratch,
// ffm_engine_predict_pair_ablated[_device] run ffm_ablate_pairs_kernel (kernels_ablate_pairs.h) and, per variant,
// field ablation's loss sum and score histogram kernels (kernels_ablate.h, gridDim.y = V + 1);
// ffm_engine_pair_ablation_read reduces the histograms on the host as ffm_engine_ablation_read does.  Nothing here
// feeds the metric channels, the keyed capture or field ablation's state, and an engine that never calls
// ffm_engine_pair_ablation_enable allocates and launches nothing of it.
// (The kernel's dynamic LDS is pred_lds_bytes(kPredLdsCap) = 12 KB at the most, like the other wave kernels'.)
// Part of engine.hip's translation unit (included inside its extern "C" block).

// ---- the variants' numbering ------------------------------------------------------------------------------
int32_t ffm_engine_pair_count(int32_t n_fields) {
  if (n_fields < 1 || n_fields > kPairFields) {
    fail(FFM_E_INVALID, "pair ablation numbers the pairs of 1 .. 64 fields, got n_fields = " + std::to_string(n_fields));
    return -1;
  }
  return pair_variants(n_fields);
}

int32_t ffm_engine_pair_index(int32_t n_fields, int32_t f, int32_t g) {
  if (ffm_engine_pair_count(n_fields) < 0) return -1;
  if (f < 0 || g < 0 || f >= n_fields || g >= n_fields) {
    fail(FFM_E_INVALID, "pair (" + std::to_string(f) + ", " + std::to_string(g) + ") names a field outside [0, n_fields)");
    return -1;
  }
  return pair_base(n_fields, std::min(f, g)) + std::max(f, g);
}

int ffm_engine_pair_fields(int32_t n_fields, int32_t v, int32_t *f, int32_t *g) {
  const int V = ffm_engine_pair_count(n_fields);
  if (V < 0) return FFM_E_INVALID;
  if (!f || !g) return fail(FFM_E_INVALID, "null output");
  if (v < 0 || v >= V)
    return fail(FFM_E_INVALID, "variant " + std::to_string(v) + " is no pair: the pairs of " + std::to_string(n_fields) +
                                   " fields are 0 .. " + std::to_string(V - 1) + " (variant " + std::to_string(V) + " is the row itself)");
  int lo = 0;  // the last f whose first pair (f, f) is at or before v
  while (lo + 1 < n_fields && pair_base(n_fields, lo + 1) + lo + 1 <= v) lo++;
  *f = lo;
  *g = v - pair_base(n_fields, lo);
  return FFM_OK;
}

// ---- the engine's share -------------------------------------------------------------------------------------
static int pair_variants_of(const ffm_engine *e) { return pair_variants(e->m.n_fields) + 1; }

// An array ffm_engine::alloc made, given back (a failed enable leaves the engine as it was).
extern "C++" {
template <typename T>
static void pair_unalloc(ffm_engine *e, T **p) {
  if (!*p) return;
  auto it = std::find(e->allocs.begin(), e->allocs.end(), static_cast<void *>(*p));
  if (it != e->allocs.end()) e->allocs.erase(it);
  (void)hipFree(*p);
  *p = nullptr;
}
}
// The V + 1 histograms: the one allocation of this file that can be tens of gigabytes.  FFM_PAIR_HIST_FAIL=1 (read
// at each call; a test hook, like FFM_TEXT_SLOT_BYTES) makes it fail as an exhausted device does, so that what
// ffm_engine_pair_ablation_enable does then can be pinned without filling a device's memory.
static int pair_hist_alloc(ffm_engine *e, unsigned long long **hist, size_t words) {
  const char *sv = std::getenv("FFM_PAIR_HIST_FAIL");
  if (sv && sv[0] == '1')
    return fail(FFM_E_NOMEM, "hipMalloc of " + std::to_string(words * sizeof(unsigned long long)) + " bytes failed: FFM_PAIR_HIST_FAIL is set");
  return e->alloc(hist, words);
}

int ffm_engine_pair_ablation_enable(ffm_engine *e, int32_t with_auc) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  const ModelDev &m = e->m;
  if (m.type != FFM_MODEL_FFM) return fail(FFM_E_UNSUPPORTED, "pair ablation is FFM only: LR and FM rows have no fields");
  if (m.n_shards > 1 || e->in_group)
    return fail(FFM_E_UNSUPPORTED, "pair ablation needs a whole model on one device (n_shards == 1, not a group's engine)");
  if (m.field_start || m.own_n || m.lin_own)
    return fail(FFM_E_UNSUPPORTED, "pair ablation needs full-length records (not a shard's compact storage)");
  if (m.n_fields > kPairFields)
    return fail(FFM_E_UNSUPPORTED, "pair ablation supports at most 64 fields: a row is one wave and its 2080 pairs are 33 registers of every lane");
  if (!ablate_pairs_fn(m.lat_fmt, m.n_factors, ablate_pairs_rounds(m.n_fields)))
    return fail(FFM_E_UNSUPPORTED, "pair ablation supports n_factors 4, 8, 16, 32 or 64 (the wave kernels' lane shapes)");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  if (int rc_e = eval_launch_pending(e)) return rc_e;
  const size_t V = static_cast<size_t>(pair_variants_of(e)), R = static_cast<size_t>(std::max(1, e->max_rows));
  int rc;
  // Everything this call has to make is made before anything of the engine changes: a failed allocation gives
  // back what the call made so far and leaves the engine -- its state and its memory -- as it was.
  const bool make_scratch = !e->pabl.out, make_hist = with_auc && !e->pabl.hist;
  float *out = nullptr;
  double *loss = nullptr, *sums = nullptr, *part = nullptr;
  unsigned long long *hist = nullptr;
  rc = FFM_OK;
  if (make_scratch && !(rc = e->alloc(&out, V * R)) && !(rc = e->alloc(&loss, V * R)) && !(rc = e->alloc(&sums, V)))
    rc = e->alloc(&part, V * (kLossParts + 1));
  if (!rc && make_hist) rc = pair_hist_alloc(e, &hist, V * kMetricWords);
  if (rc) {
    pair_unalloc(e, &out);
    pair_unalloc(e, &loss);
    pair_unalloc(e, &sums);
    pair_unalloc(e, &part);
    pair_unalloc(e, &hist);
    return rc;
  }
  if (make_scratch) {
    e->pabl.out = out;
    e->pabl.loss = loss;
    e->pabl.sums = sums;
    e->pabl.part = part;
    HIP_TRY(hipMemsetAsync(e->pabl.part, 0, sizeof(double) * V * (kLossParts + 1), e->stream));
  }
  if (make_hist) e->pabl.hist = hist;
  if (with_auc && !e->pabl.auc)  // (collection that turns on starts from zero, collection that stays on keeps its counts)
    HIP_TRY(hipMemsetAsync(e->pabl.hist, 0, sizeof(unsigned long long) * V * kMetricWords, e->stream));
  e->pabl.auc = with_auc != 0;
  e->pabl.on = true;
  return FFM_OK;
}

// The launches, on a block in device memory; row_cap as launch_row_kernel takes it.  out / loss_sum_out: device
// arrays of the variants' scores and loss sums, or null (the scores then stay in the engine's scratch).
static int pair_ablate_core(ffm_engine *e, const Rows &rows, int row_cap, int32_t output_prob, float *out, double *loss_sum_out) {
  const ModelDev &m = e->m;
  const int V = pair_variants_of(e), n_rows = rows.n_rows;
  float *const score = out ? out : e->pabl.out;
  if (n_rows > 0) {
    if (row_cap <= 0) row_cap = e->max_row_nnz;
    const int lds_cap = std::min(row_cap, kPredLdsCap);
    hipLaunchKernelGGL(ablate_pairs_fn(m.lat_fmt, m.n_factors, ablate_pairs_rounds(m.n_fields)), dim3(cdiv(n_rows, kPredRows)),
                       dim3(64 * kPredRows), pred_lds_bytes(lds_cap), e->stream, m, rows, e->d_err, row_cap, lds_cap, score,
                       e->pabl.loss, e->max_rows, output_prob);
    if (rows.label && e->pabl.auc)
      hipLaunchKernelGGL(ablate_hist_kernel, dim3(cdiv(n_rows, kMetricThreads), V), dim3(kMetricThreads), 0, e->stream, n_rows,
                         score, output_prob, rows.label, e->pabl.hist);
  }
  if (loss_sum_out) {
    if (rows.label && n_rows > 0)
      hipLaunchKernelGGL(ablate_loss_sum_kernel, dim3(loss_grid(n_rows), V), dim3(256), 0, e->stream, n_rows, e->pabl.loss,
                         e->max_rows, loss_sum_out, e->pabl.part);
    else
      HIP_TRY(hipMemsetAsync(loss_sum_out, 0, sizeof(double) * V, e->stream));
  }
  HIP_TRY(hipGetLastError());
  return FFM_OK;
}

static int pair_ablate_ready(ffm_engine *e) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  if (!e->pabl.on) return fail(FFM_E_INVALID, "pair ablation is off (ffm_engine_pair_ablation_enable)");
  return FFM_OK;
}

int ffm_engine_predict_pair_ablated_device(ffm_engine *e, int32_t n_rows, int32_t nnz, const int32_t *row_ptr,
                                           const int32_t *field, const int32_t *feat, const float *val, const int32_t *label,
                                           int32_t output_prob, float *out, double *loss_sum_out) {
  int rc = pair_ablate_ready(e);
  if (rc) return rc;
  if ((rc = check_block(e, n_rows, nnz, row_ptr, field, feat, val))) return rc;
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  return pair_ablate_core(e, Rows{n_rows, nnz, row_ptr, field, feat, val, label}, 0, output_prob, out, loss_sum_out);
}

int ffm_engine_predict_pair_ablated(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr, const int32_t *field,
                                    const int32_t *feat, const float *val, const int32_t *label, int32_t output_prob,
                                    float *out, double *loss_sum_out) {
  int rc = pair_ablate_ready(e);
  if (rc) return rc;
  Rows dev{};
  int row_cap = 0;
  if ((rc = stage_block(e, n_rows, row_ptr, field, feat, val, label, &dev, &row_cap))) return rc;
  const size_t V = static_cast<size_t>(pair_variants_of(e));
  if ((rc = pair_ablate_core(e, dev, row_cap, output_prob, nullptr, label ? e->pabl.sums : nullptr))) return rc;
  if (out && n_rows > 0)
    HIP_TRY(hipMemcpyAsync(out, e->pabl.out, sizeof(float) * V * n_rows, hipMemcpyDeviceToHost, e->stream));
  if (loss_sum_out) {
    if (label && n_rows > 0) HIP_TRY(hipMemcpyAsync(loss_sum_out, e->pabl.sums, sizeof(double) * V, hipMemcpyDeviceToHost, e->stream));
    else std::fill(loss_sum_out, loss_sum_out + V, 0.0);
  }
  return check_device_errors(e);
}

int ffm_engine_pair_ablation_read(ffm_engine *e, int32_t reset, ffm_metrics *out) {
  int rc = pair_ablate_ready(e);
  if (rc) return rc;
  if (!out) return fail(FFM_E_INVALID, "null output");
  if (!e->pabl.auc) return fail(FFM_E_INVALID, "pair ablation was enabled without histograms (with_auc == 0)");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  if (int rc_e = eval_launch_pending(e)) return rc_e;
  const int V = pair_variants_of(e);
  const size_t bytes = kMetricWords * sizeof(unsigned long long);
  std::vector<unsigned long long> h;
  try { h.assign(kMetricWords, 0ull); } catch (const std::bad_alloc &) { return fail(FFM_E_NOMEM, "host allocation failed"); }
  for (int v = 0; v < V; v++) {  // (one histogram at a time: 16 MiB of host memory, not 16 MiB per pair)
    unsigned long long *const hist = e->pabl.hist + static_cast<size_t>(v) * kMetricWords;
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
