// engine_ablate.h -- field ablation, pair ablation and the pruning curve (include/ffm_engine.h "Field ablation", "Pair
// ablation", "Pruning curve"): enable makes a kind's variant-major scratch (ffm_engine::abl, ::pabl, ::cabl), predict
// runs its wave kernel -- ffm_ablate_wave_kernel (kernels_ablate.h), ffm_ablate_pairs_kernel (kernels_ablate_pairs.h)
// or ffm_curve_wave_kernel (kernels_curve.h) -- and, per variant, the loss sum and the score histogram
// (kernels_ablate.h, gridDim.y = the variants); read reduces the histograms on the host as ffm_engine_metrics_read
// does.  The kinds differ in what an AblateKind says and, for the curve, in the table and cuts its enable takes; the
// pairs' numbering (host arithmetic, no device) is here too.  Nothing here feeds the metric channels, the keyed
// capture or another kind's state, and an engine that never calls an enable allocates and launches nothing of it.
// (A kernel's dynamic LDS is curve_lds_bytes(kPredLdsCap) = 16 KB at the most: within the default limit, so
// opt_in_lds has nothing to ask for.)
// Part of engine.hip's translation unit (included inside its extern "C" block).

// ---- the pairs' numbering ---------------------------------------------------------------------------------
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

// ---- what a kind is ---------------------------------------------------------------------------------------
struct AblateKind {
  ffm_engine::AblateSet ffm_engine::*set;
  int (*variants)(const ffm_engine &e);  // the row itself included; the curve's: of the cuts in force
  bool (*served)(const ModelDev &m);     // there is a wave kernel for the model's shape
  // the kind's wave kernel on a block: score / loss variant-major, loss with the stride e->max_rows
  void (*launch)(const ffm_engine *e, const Rows &rows, int row_cap, int lds_cap, float *score, double *loss, int output_prob);
  const char *noun, *prefix;  // "field ablation"; the entry points are ffm_engine_<prefix>_enable, _read
  const char *why_64;         // the reason behind "at most 64 fields"
  const char *fail_env;       // the failure hook of the histograms' allocation (ablate_enable)
};
static int field_variants(const ffm_engine &e) { return e.m.n_fields + 1; }
static int pair_variants_all(const ffm_engine &e) { return pair_variants(e.m.n_fields) + 1; }
static int curve_variants(const ffm_engine &e) { return e.cabl.variants; }  // (n_cuts + 1: what its scratch holds)
static AblateWaveFn field_kernel(const ModelDev &m) { return ablate_wave_fn(m.lat_fmt, m.n_factors); }
static AblateWaveFn pair_kernel(const ModelDev &m) { return ablate_pairs_fn(m.lat_fmt, m.n_factors, ablate_pairs_rounds(m.n_fields)); }
static bool field_served(const ModelDev &m) { return field_kernel(m) != nullptr; }
static bool pair_served(const ModelDev &m) { return pair_kernel(m) != nullptr; }
static bool curve_served(const ModelDev &m) { return curve_wave_fn(m.lat_fmt, m.n_factors) != nullptr; }
static void ablate_wave_launch(AblateWaveFn fn, const ffm_engine *e, const Rows &rows, int row_cap, int lds_cap, float *score,
                               double *loss, int output_prob) {
  hipLaunchKernelGGL(fn, dim3(cdiv(rows.n_rows, kPredRows)), dim3(64 * kPredRows), pred_lds_bytes(lds_cap), e->stream, e->m, rows,
                     e->d_err, row_cap, lds_cap, score, loss, e->max_rows, output_prob);
}
static void field_launch(const ffm_engine *e, const Rows &rows, int row_cap, int lds_cap, float *score, double *loss, int output_prob) {
  ablate_wave_launch(field_kernel(e->m), e, rows, row_cap, lds_cap, score, loss, output_prob);
}
static void pair_launch(const ffm_engine *e, const Rows &rows, int row_cap, int lds_cap, float *score, double *loss, int output_prob) {
  ablate_wave_launch(pair_kernel(e->m), e, rows, row_cap, lds_cap, score, loss, output_prob);
}
static void curve_launch(const ffm_engine *e, const Rows &rows, int row_cap, int lds_cap, float *score, double *loss, int output_prob) {
  hipLaunchKernelGGL(curve_wave_fn(e->m.lat_fmt, e->m.n_factors), dim3(cdiv(rows.n_rows, kPredRows)), dim3(64 * kPredRows),
                     curve_lds_bytes(lds_cap), e->stream, e->m, rows, e->d_err, row_cap, lds_cap, score, loss, e->max_rows, output_prob,
                     CurveDev{e->d_curve_level, e->d_curve_cut, e->cabl.variants - 1});
}
static const AblateKind kFieldAblation = {&ffm_engine::abl, field_variants, field_served, field_launch, "field ablation", "ablation",
                                          "a row is one wave and a variant one lane of it", "FFM_FIELD_HIST_FAIL"};
static const AblateKind kPairAblation = {&ffm_engine::pabl, pair_variants_all, pair_served, pair_launch, "pair ablation", "pair_ablation",
                                         "a row is one wave and its 2080 pairs are 33 registers of every lane", "FFM_PAIR_HIST_FAIL"};
static const AblateKind kPairCurve = {&ffm_engine::cabl, curve_variants, curve_served, curve_launch, "the pruning curve", "pair_curve",
                                      "a level table row is a mask word, and a variant one lane of a row's wave", "FFM_CURVE_HIST_FAIL"};

// What every kind asks of an engine, with the kind's noun in the messages.
static int ablate_supported(const AblateKind &k, ffm_engine *e) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  const ModelDev &m = e->m;
  const std::string noun = k.noun;
  if (m.type != FFM_MODEL_FFM) return fail(FFM_E_UNSUPPORTED, noun + " is FFM only: LR and FM rows have no fields");
  if (m.n_shards > 1 || e->in_group)
    return fail(FFM_E_UNSUPPORTED, noun + " needs a whole model on one device (n_shards == 1, not a group's engine)");
  if (m.field_start || m.own_n || m.lin_own)
    return fail(FFM_E_UNSUPPORTED, noun + " needs full-length records (not a shard's compact storage)");
  if (m.n_fields > kPairFields) return fail(FFM_E_UNSUPPORTED, noun + " supports at most 64 fields: " + k.why_64);
  if (!k.served(m))
    return fail(FFM_E_UNSUPPORTED, noun + " supports n_factors 4, 8, 16, 32 or 64 (the wave kernels' lane shapes)");
  return FFM_OK;
}

// n_variants: what the kind's scratch is to hold from now on -- k.variants(e) for the kinds whose count is the
// model's; the curve's changes with its cuts, and a set made for another count is replaced (scratch and histograms:
// the new histograms start from zero).
// (ablate_make: the part behind ablate_supported, which the curve's enable has already asked.)
static int ablate_make(const AblateKind &k, ffm_engine *e, int32_t with_auc, int n_variants) {
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  if (int rc_e = eval_launch_pending(e)) return rc_e;
  ffm_engine::AblateSet &s = e->*k.set;
  const size_t V = static_cast<size_t>(n_variants), R = static_cast<size_t>(std::max(1, e->max_rows));
  // Everything this call has to make is made before anything of the engine changes: a failed allocation gives
  // back what the call made so far and leaves the engine -- its state and its memory -- as it was.
  const bool resize = s.out && s.variants != n_variants;
  const bool make_scratch = !s.out || resize, make_hist = with_auc && (!s.hist || resize);
  ffm_engine::AblateSet made;
  int rc = FFM_OK;
  if (make_scratch && !(rc = e->alloc(&made.out, V * R)) && !(rc = e->alloc(&made.loss, V * R)) && !(rc = e->alloc(&made.sums, V)))
    rc = e->alloc(&made.part, V * (kLossParts + 1));
  if (!rc && make_hist) {
    // The one allocation here that can be tens of gigabytes.  FFM_FIELD_HIST_FAIL=1 / FFM_PAIR_HIST_FAIL=1 /
    // FFM_CURVE_HIST_FAIL=1 (read at each call; a test hook, like FFM_TEXT_SLOT_BYTES) makes it fail as an exhausted
    // device does, so that what this function does then can be pinned without filling a device's memory.
    const char *sv = std::getenv(k.fail_env);
    if (sv && sv[0] == '1')
      rc = fail(FFM_E_NOMEM, "hipMalloc of " + std::to_string(V * kMetricWords * sizeof(unsigned long long)) + " bytes failed: " + k.fail_env + " is set");
    else
      rc = e->alloc(&made.hist, V * kMetricWords);
  }
  if (rc) {
    e->release(&made.out);
    e->release(&made.loss);
    e->release(&made.sums);
    e->release(&made.part);
    e->release(&made.hist);
    return rc;
  }
  if (resize) {  // (hipFree waits for what still reads the old arrays)
    e->release(&s.out);
    e->release(&s.loss);
    e->release(&s.sums);
    e->release(&s.part);
    e->release(&s.hist);
    s.auc = false;
  }
  if (make_scratch) {
    s.out = made.out;
    s.loss = made.loss;
    s.sums = made.sums;
    s.part = made.part;
    HIP_TRY(hipMemsetAsync(s.part, 0, sizeof(double) * V * (kLossParts + 1), e->stream));
  }
  if (make_hist) s.hist = made.hist;
  if (with_auc && !s.auc)  // (collection that turns on starts from zero, collection that stays on keeps its counts)
    HIP_TRY(hipMemsetAsync(s.hist, 0, sizeof(unsigned long long) * V * kMetricWords, e->stream));
  s.auc = with_auc != 0;
  s.variants = n_variants;
  s.on = true;
  return FFM_OK;
}
static int ablate_enable(const AblateKind &k, ffm_engine *e, int32_t with_auc, int n_variants) {
  if (int rc_s = ablate_supported(k, e)) return rc_s;
  return ablate_make(k, e, with_auc, n_variants);
}

// ---- the pruning curve's own part of its enable: what a table and its cuts must be, and their way to HBM ------
static int curve_enable(ffm_engine *e, const uint16_t *level, int32_t n_fields, const int32_t *cut, int32_t n_cuts, int32_t with_auc) {
  const AblateKind &k = kPairCurve;
  if (int rc_s = ablate_supported(k, e)) return rc_s;
  const ModelDev &m = e->m;
  // ---- a refused table or list leaves the previous ones in force
  if (!level || !cut) return fail(FFM_E_INVALID, "null level table or cuts");
  if (n_fields != m.n_fields)
    return fail(FFM_E_INVALID, "the level table is for " + std::to_string(n_fields) + " fields, the engine has " + std::to_string(m.n_fields));
  if (n_cuts < 1 || n_cuts > kCurveCuts)
    return fail(FFM_E_INVALID, "the pruning curve takes 1 .. 64 cuts a pass (a cut is one lane of a row's wave), got n_cuts = " + std::to_string(n_cuts));
  for (int c = 0; c < n_cuts; c++)
    if (cut[c] < 0 || cut[c] > kCurveLevelMax)
      return fail(FFM_E_INVALID, "cut[" + std::to_string(c) + "] = " + std::to_string(cut[c]) + " lies outside [0, 65536]");
  for (int f = 0; f < n_fields; f++)
    for (int g = 0; g < f; g++)
      if (level[f * n_fields + g] != level[g * n_fields + f])
        return fail(FFM_E_INVALID, "the level table is not symmetric: level[" + std::to_string(f) + "][" + std::to_string(g) + "] = " +
                                       std::to_string(level[f * n_fields + g]) + ", level[" + std::to_string(g) + "][" + std::to_string(f) +
                                       "] = " + std::to_string(level[g * n_fields + f]));
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  // The table and the cuts go into arrays of their own, made and filled by this call and waited for, before anything
  // of the engine changes: nothing of the caller's is read after this returns, the kernels queued so far go on
  // reading the previous arrays, and a failure up to here gives the new ones back and leaves the engine as it was.
  unsigned short *d_level = nullptr;
  int *d_cut = nullptr;
  int rc = e->alloc(&d_level, static_cast<size_t>(kCurveFields) * kCurveFields);
  if (!rc) rc = e->alloc(&d_cut, static_cast<size_t>(kCurveCuts));
  if (!rc) {
    hipError_t err = hipMemcpyAsync(d_level, level, sizeof(uint16_t) * n_fields * n_fields, hipMemcpyHostToDevice, e->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(d_cut, cut, sizeof(int32_t) * n_cuts, hipMemcpyHostToDevice, e->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    if (err != hipSuccess) rc = fail(FFM_E_DEVICE, std::string("copying the level table and the cuts failed: ") + hipGetErrorString(err));
  }
  if (!rc) rc = ablate_make(k, e, with_auc, n_cuts + 1);  // (its failed allocation leaves the engine as it was, too)
  if (rc) {
    e->release(&d_level);
    e->release(&d_cut);
    return rc;
  }
  // in force from here on, with the scratch ablate_make has just sized for them (the curve's count is the scratch's
  // own, AblateSet::variants); hipFree waits for what still reads the previous arrays
  e->release(&e->d_curve_level);
  e->release(&e->d_curve_cut);
  e->d_curve_level = d_level;
  e->d_curve_cut = d_cut;
  return FFM_OK;
}

// The launches, on a block in device memory; row_cap as launch_row_kernel takes it.  out / loss_sum_out: device
// arrays of the variants' scores and loss sums, or null (the scores then stay in the engine's scratch).
static int ablate_core(const AblateKind &k, ffm_engine *e, const Rows &rows, int row_cap, int32_t output_prob, float *out,
                       double *loss_sum_out) {
  const ffm_engine::AblateSet &s = e->*k.set;
  const int V = k.variants(*e), n_rows = rows.n_rows;
  float *const score = out ? out : s.out;
  if (n_rows > 0) {
    if (row_cap <= 0) row_cap = e->max_row_nnz;
    const int lds_cap = std::min(row_cap, kPredLdsCap);
    k.launch(e, rows, row_cap, lds_cap, score, s.loss, output_prob);
    if (rows.label && s.auc)
      hipLaunchKernelGGL(ablate_hist_kernel, dim3(cdiv(n_rows, kMetricThreads), V), dim3(kMetricThreads), 0, e->stream, n_rows,
                         score, output_prob, rows.label, s.hist);
  }
  if (loss_sum_out) {
    if (rows.label && n_rows > 0)
      hipLaunchKernelGGL(ablate_loss_sum_kernel, dim3(loss_grid(n_rows), V), dim3(256), 0, e->stream, n_rows, s.loss, e->max_rows,
                         loss_sum_out, s.part);
    else
      HIP_TRY(hipMemsetAsync(loss_sum_out, 0, sizeof(double) * V, e->stream));
  }
  HIP_TRY(hipGetLastError());
  return FFM_OK;
}

static int ablate_ready(const AblateKind &k, ffm_engine *e) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  if (!(e->*k.set).on) return fail(FFM_E_INVALID, std::string(k.noun) + " is off (ffm_engine_" + k.prefix + "_enable)");  return FFM_OK;
}

static int ablate_predict_device(const AblateKind &k, ffm_engine *e, int32_t n_rows, int32_t nnz, const int32_t *row_ptr,
                                 const int32_t *field, const int32_t *feat, const float *val, const int32_t *label,
                                 int32_t output_prob, float *out, double *loss_sum_out) {
  int rc = ablate_ready(k, e);
  if (rc) return rc;
  MASK_REFUSE(e, k.noun);  // (its variants are the whole model's: include/ffm_engine.h "Pair masks")
  if ((rc = check_block(e, n_rows, nnz, row_ptr, field, feat, val))) return rc;
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  return ablate_core(k, e, Rows{n_rows, nnz, row_ptr, field, feat, val, label}, 0, output_prob, out, loss_sum_out);
}

static int ablate_predict(const AblateKind &k, ffm_engine *e, int32_t n_rows, const int32_t *row_ptr, const int32_t *field,
                          const int32_t *feat, const float *val, const int32_t *label, int32_t output_prob, float *out,
                          double *loss_sum_out) {
  int rc = ablate_ready(k, e);
  if (rc) return rc;
  MASK_REFUSE(e, k.noun);  // (its variants are the whole model's: include/ffm_engine.h "Pair masks")
  Rows dev{};
  int row_cap = 0;
  if ((rc = stage_block(e, n_rows, row_ptr, field, feat, val, label, &dev, &row_cap))) return rc;
  const ffm_engine::AblateSet &s = e->*k.set;
  const size_t V = static_cast<size_t>(k.variants(*e));
  if ((rc = ablate_core(k, e, dev, row_cap, output_prob, nullptr, label ? s.sums : nullptr))) return rc;
  if (out && n_rows > 0) HIP_TRY(hipMemcpyAsync(out, s.out, sizeof(float) * V * n_rows, hipMemcpyDeviceToHost, e->stream));
  if (loss_sum_out) {
    if (label && n_rows > 0) HIP_TRY(hipMemcpyAsync(loss_sum_out, s.sums, sizeof(double) * V, hipMemcpyDeviceToHost, e->stream));
    else std::fill(loss_sum_out, loss_sum_out + V, 0.0);
  }
  return check_device_errors(e);
}

static int ablate_read(const AblateKind &k, ffm_engine *e, int32_t reset, ffm_metrics *out) {
  int rc = ablate_ready(k, e);
  if (rc) return rc;
  if (!out) return fail(FFM_E_INVALID, "null output");
  const ffm_engine::AblateSet &s = e->*k.set;
  if (!s.auc) return fail(FFM_E_INVALID, std::string(k.noun) + " was enabled without histograms (with_auc == 0)");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  if (int rc_e = eval_launch_pending(e)) return rc_e;
  const int V = k.variants(*e);
  const size_t bytes = kMetricWords * sizeof(unsigned long long);
  std::vector<unsigned long long> h;
  try { h.assign(kMetricWords, 0ull); } catch (const std::bad_alloc &) { return fail(FFM_E_NOMEM, "host allocation failed"); }
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the counters are 64-bit");
  for (int v = 0; v < V; v++) {  // (one histogram at a time: 16 MiB of host memory, not 16 MiB per variant)
    unsigned long long *const hist = s.hist + static_cast<size_t>(v) * kMetricWords;
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

// ---- the exports ------------------------------------------------------------------------------------------
int ffm_engine_ablation_enable(ffm_engine *e, int32_t with_auc) {
  return ablate_enable(kFieldAblation, e, with_auc, e ? field_variants(*e) : 0);
}
int ffm_engine_pair_ablation_enable(ffm_engine *e, int32_t with_auc) {
  return ablate_enable(kPairAblation, e, with_auc, e && e->m.n_fields <= kPairFields ? pair_variants_all(*e) : 0);
}
int ffm_engine_pair_curve_enable(ffm_engine *e, const uint16_t *level, int32_t n_fields, const int32_t *cut, int32_t n_cuts,
                                 int32_t with_auc) {
  return curve_enable(e, level, n_fields, cut, n_cuts, with_auc);
}
int ffm_engine_ablation_read(ffm_engine *e, int32_t reset, ffm_metrics *out) { return ablate_read(kFieldAblation, e, reset, out); }
int ffm_engine_pair_ablation_read(ffm_engine *e, int32_t reset, ffm_metrics *out) { return ablate_read(kPairAblation, e, reset, out); }
int ffm_engine_pair_curve_read(ffm_engine *e, int32_t reset, ffm_metrics *out) { return ablate_read(kPairCurve, e, reset, out); }
int ffm_engine_predict_ablated_device(ffm_engine *e, int32_t n_rows, int32_t nnz, const int32_t *row_ptr, const int32_t *field,
                                      const int32_t *feat, const float *val, const int32_t *label, int32_t output_prob,
                                      float *out, double *loss_sum_out) {
  return ablate_predict_device(kFieldAblation, e, n_rows, nnz, row_ptr, field, feat, val, label, output_prob, out, loss_sum_out);
}
int ffm_engine_predict_pair_ablated_device(ffm_engine *e, int32_t n_rows, int32_t nnz, const int32_t *row_ptr,
                                           const int32_t *field, const int32_t *feat, const float *val, const int32_t *label,
                                           int32_t output_prob, float *out, double *loss_sum_out) {
  return ablate_predict_device(kPairAblation, e, n_rows, nnz, row_ptr, field, feat, val, label, output_prob, out, loss_sum_out);
}
int ffm_engine_predict_ablated(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr, const int32_t *field,
                               const int32_t *feat, const float *val, const int32_t *label, int32_t output_prob, float *out,
                               double *loss_sum_out) {
  return ablate_predict(kFieldAblation, e, n_rows, row_ptr, field, feat, val, label, output_prob, out, loss_sum_out);
}
int ffm_engine_predict_pair_ablated(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr, const int32_t *field,
                                    const int32_t *feat, const float *val, const int32_t *label, int32_t output_prob,
                                    float *out, double *loss_sum_out) {
  return ablate_predict(kPairAblation, e, n_rows, row_ptr, field, feat, val, label, output_prob, out, loss_sum_out);
}
int ffm_engine_predict_pair_curve_device(ffm_engine *e, int32_t n_rows, int32_t nnz, const int32_t *row_ptr, const int32_t *field,
                                         const int32_t *feat, const float *val, const int32_t *label, int32_t output_prob,
                                         float *out, double *loss_sum_out) {
  return ablate_predict_device(kPairCurve, e, n_rows, nnz, row_ptr, field, feat, val, label, output_prob, out, loss_sum_out);
}
int ffm_engine_predict_pair_curve(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr, const int32_t *field, const int32_t *feat,
                                  const float *val, const int32_t *label, int32_t output_prob, float *out, double *loss_sum_out) {
  return ablate_predict(kPairCurve, e, n_rows, row_ptr, field, feat, val, label, output_prob, out, loss_sum_out);
}
