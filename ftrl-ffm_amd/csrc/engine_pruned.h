// engine_pruned.h -- pruned serving tables (include/ffm_engine.h "Pruned serving tables"): what
// ffm_engine_create_pruned checks before a device is asked for, the layout on the host, the table's small arrays in
// HBM, and the launches of kernels_pruned.h that engine_create.h (contents at create), engine_serve.h (full-length
// rows in and out, ffm_engine_pack_weights) and engine_step.h (rows) dispatch to on such an engine.
// Part of engine.hip's translation unit (included inside its extern "C" block).

// base_out[n_fields + 1] of checked words and ranges; the table's slots are base_out[n_fields].
static void pruned_layout(const uint64_t *keep, int32_t n_fields, const int32_t *field_start, int64_t *base_out) {
  base_out[0] = 0;
  for (int f = 0; f < n_fields; f++)
    base_out[f + 1] = base_out[f] + (static_cast<int64_t>(field_start[f + 1]) - field_start[f]) * __builtin_popcountll(keep[f]);
}

// The mask and the ranges, without a device: n_feats < 0 leaves the ranges' end open (ffm_engine_pruned_layout_host).
static int pruned_check(const uint64_t *keep, int32_t n_fields, const int32_t *field_start, int64_t n_feats) {
  const std::string noun = "a pruned serving table";
  if (!keep) return fail(FFM_E_INVALID, noun + " needs its pair mask (keep == NULL)");
  if (n_fields < 1) return fail(FFM_E_INVALID, "n_fields must be positive");
  if (n_fields > kMaskFields) return fail(FFM_E_UNSUPPORTED, noun + " supports at most 64 fields: a field's partners are one 64-bit word");
  if (int rc_w = pair_mask_words_check(keep, n_fields)) return rc_w;
  if (!field_start)
    return fail(FFM_E_INVALID, noun + " needs per-field id ranges (field_start == NULL): without them an id may appear under any field");
  bool ok = field_start[0] == 0 && (n_feats < 0 || field_start[n_fields] == n_feats);
  for (int f = 0; f < n_fields; f++) ok = ok && field_start[f] <= field_start[f + 1];
  if (!ok) return fail(FFM_E_INVALID, "field_start must ascend from 0 to n_feats");
  int64_t base[kMaskFields + 1];
  pruned_layout(keep, n_fields, field_start, base);
  if (base[n_fields] >= (1ll << 32))
    return fail(FFM_E_UNSUPPORTED, noun + " of " + std::to_string(base[n_fields]) + " slots: a slot number is 32 bits (fewer than 2^32 slots)");
  return FFM_OK;
}

int ffm_engine_pruned_layout_host(const uint64_t *keep, int32_t n_fields, const int32_t *field_start, int64_t *base_out) {
  if (!base_out) return fail(FFM_E_INVALID, "null output");
  if (int rc = pruned_check(keep, n_fields, field_start, -1)) return rc;
  pruned_layout(keep, n_fields, field_start, base_out);
  return FFM_OK;
}

int ffm_engine_create_pruned(const ffm_engine_config *cfg, const uint64_t *keep, int32_t n_fields, ffm_engine **out) {
  if (!cfg || !out) return fail(FFM_E_INVALID, "null config or output pointer");
  *out = nullptr;
  if (cfg->flags & FFM_FLAG_SERVE_F8)
    return fail(FFM_E_UNSUPPORTED, "a pruned serving table is fp32 or fp16 (FFM_FLAG_SERVE_F32 / _F16): FFM_FLAG_SERVE_F8, the f8 "
                                   "format, has no pruned layout");
  if (!(cfg->flags & (FFM_FLAG_SERVE_F32 | FFM_FLAG_SERVE_F16)))
    return fail(FFM_E_INVALID, "a pruned serving table needs a serving config: FFM_FLAG_SERVE_F32 or FFM_FLAG_SERVE_F16");
  if (int rc_s = serve_create_check(cfg)) return rc_s;  // (both flags; LR / FM; shards; n_factors; max_row_nnz)
  if (n_fields != cfg->n_fields)
    return fail(FFM_E_INVALID, "the mask is for " + std::to_string(n_fields) + " fields, the engine has " + std::to_string(cfg->n_fields));
  if (int rc_p = pruned_check(keep, n_fields, cfg->field_start, cfg->n_feats)) return rc_p;
  return engine_create(cfg, keep, out);
}

// ---- create's steps on a pruned engine (engine_create.h) ------------------------------------------------------

// The table's size, behind plan_model (which copied and checked cfg->field_start).
static int pruned_plan(ffm_engine *e) {
  int64_t base[kMaskFields + 1];
  pruned_layout(e->pair_mask, e->m.n_fields, e->field_start.data(), base);
  e->pruned_slots = base[e->m.n_fields];
  return FFM_OK;
}

// The mask words, the id ranges and the bases in HBM.
static int pruned_tables(ffm_engine *e) {
  const int F = e->m.n_fields;
  int64_t base[kMaskFields + 1];
  pruned_layout(e->pair_mask, F, e->field_start.data(), base);
  std::vector<unsigned long long> words(e->pair_mask, e->pair_mask + kMaskFields);
  std::vector<unsigned> base32(base, base + F + 1);  // (below 2^32: pruned_check)
  unsigned long long *d_keep = nullptr;
  int *d_start = nullptr;
  unsigned *d_base = nullptr;
  int rc;
  if ((rc = upload(e, words, &d_keep)) || (rc = upload(e, e->field_start, &d_start)) || (rc = upload(e, base32, &d_base))) return rc;
  e->pd = PrunedDev{d_keep, d_start, d_base};
  return FFM_OK;
}

static int pruned_grid(int64_t items) {
  return static_cast<int>(std::min<int64_t>(2048, std::max<int64_t>(1, (items + kPrunedThreads - 1) / kPrunedThreads)));
}

static void pruned_launch_init(ffm_engine *e) {
  const int64_t items = std::max<int64_t>(e->pruned_slots * e->m.n_factors, e->m.n_feats);
  hipLaunchKernelGGL(pruned_init_kernel, dim3(pruned_grid(items)), dim3(kPrunedThreads), 0, e->stream, e->m, e->pd, e->cfg.init_mean,
                     e->cfg.init_stddev, e->cfg.seed);
}

// ---- full-length fp32 rows in e->d_stage <-> the table (engine_serve.h) -----------------------------------------
// nf rows: features ids[j] (device), or feat0 + j when ids is null.
static void pruned_launch_copy(ffm_engine *e, const int *ids, int64_t feat0, int64_t nf, bool to_host) {
  hipLaunchKernelGGL(pruned_rows_copy_kernel, dim3(pruned_grid(nf * e->logical_len)), dim3(kPrunedThreads), 0, e->stream, e->m, e->pd,
                     e->d_stage, ids, feat0, nf, to_host ? 1 : 0);
}

// ---- ffm_engine_pack_weights into a pruned table: on dst's stream, behind the clearing of dst->d_pack ---------------
static void pruned_launch_pack(ffm_engine *dst, ffm_engine *src, int cus) {
  const ModelDev &m = dst->m;
  int widest = 0;  // the longest pruned row, in slots
  for (int f = 0; f < m.n_fields; f++) widest = std::max(widest, __builtin_popcountll(dst->pair_mask[f]));
  const int row4 = std::max(1, widest * (m.n_factors / 4));
  int G = 0;  // lanes per feature of the kernel chosen
  const ServePackPrunedFn fn = serve_pack_pruned_fn(m.lat_fmt, m.n_factors, row4, &G);
  const int grid = std::min(std::max(1, cus) * 8, pruned_grid(static_cast<int64_t>(m.n_feats) * G));
  hipLaunchKernelGGL(fn, dim3(grid), dim3(kPrunedThreads), 0, dst->stream, src->m, m, dst->pd, dst->d_pack);
}
