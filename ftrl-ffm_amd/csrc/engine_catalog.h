// engine_catalog.h -- request contexts against a whole id range of one field (include/ffm_engine.h "Scoring a
// catalogue" and "... the best K"; kernels_catalog.h, kernels_catalog_topk.h): what the entry points check, the buffers
// they grow, and the launches -- the engine's own row kernel over the contexts (base), catalog_u_kernel, then either
// catalog_gemm_kernel per 128 requests or catalog_topk_kernel per 32 RT requests and catalog_topk_merge_kernel.
// The same launches serve a table of items of several entries ("... items of several entries",
// kernels_catalog_items.h): S_c per item first, U towards every slot's field, the kernels over CatalogItemSrc -- and a
// table whose last slots are dictionary slots ("... dictionary slots", kernels_catalog_dict.h): the dictionary slots' U
// and partial scores between U and the kernels, which then run over CatalogDictSrc.
// Per-request item lists ("... per-request item lists", kernels_catalog_lists.h) share the base, the table's checks and
// the staging, and have three launches of their own: catalog_lists_launch, at the end of this file.
// Part of engine.hip's translation unit (included inside its extern "C" block).

// The engines every call of this file refuses, by name; what: "score_catalog", "score_items", "score_item_lists".
static int catalog_engine_check(ffm_engine *e, const char *what) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  if (!serving(e))
    return fail(FFM_E_UNSUPPORTED, std::string(what) + " needs a serving engine (FFM_FLAG_SERVE_F32 / _F16): "
                                                       "ffm_engine_pack_weights copies a training engine's weights into one");
  F8_REFUSE(e, what);
  PRUNED_REFUSE(e, what);
  MASK_REFUSE(e, what);
  if (e->norm_rows_on)
    return fail(FFM_E_INVALID, std::string(what) + " is not available on an engine with FFM_FLAG_NORM_ROWS: a candidate would change "
                                                   "the scale of its context's terms");
  if (e->in_group || e->m.n_shards > 1)
    return fail(FFM_E_UNSUPPORTED, std::string(what) + " is not available on a group's or a shard's engine: it reads one whole table");
  return FFM_OK;
}

static int catalog_check(ffm_engine *e, int32_t n_req, int32_t cand_field, int32_t cand_first, int32_t n_cand) {
  if (int rc = catalog_engine_check(e, "score_catalog")) return rc;
  if (n_req < 0 || n_cand < 0) return fail(FFM_E_INVALID, "negative n_req / n_cand");
  if (cand_field < 0 || cand_field >= e->m.n_fields)
    return fail(FFM_E_INVALID, "cand_field " + std::to_string(cand_field) + " lies outside [0, n_fields)");
  if (cand_first < 0 || static_cast<int64_t>(cand_first) + n_cand > e->m.n_feats)
    return fail(FFM_E_INVALID, "the candidate range [cand_first, cand_first + n_cand) lies outside [0, n_feats]");
  if (n_req > e->max_rows) return fail(FFM_E_CAPACITY, "more requests than max_batch_rows");
  return FFM_OK;
}
// ... and of the two calls that write the whole matrix
static int catalog_matrix_check(int32_t n_req, int32_t n_cand) {
  if (static_cast<int64_t>(n_req) * n_cand > 2147483647ll)
    return fail(FFM_E_CAPACITY, "n_req * n_cand exceeds 2^31 - 1 scores: split the range");
  return FFM_OK;
}
// Behind the checks, before anything is queued.
static int catalog_ready(ffm_engine *e) {
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  return eval_launch_pending(e);
}

// The requests in whole tiles of their launches: 128 per launch, the last one 32, 64 or 128.
static int catalog_rows(int n_req) {
  const int rest = n_req % 128;
  return n_req - rest + (rest ? kCatTile * catalog_rt(cdiv(rest, kCatTile)) : 0);
}

// The columns of a call when they are items of several entries (kernels_catalog_items.h) and not a field's id range:
// the slots by value, feat[n_items][slots.n] in device memory.
struct ItemTable {
  CatalogItemSlots slots;
  const int32_t *feat;
  int32_t n_items;
};

// An item table whose last slots are dictionary slots (kernels_catalog_dict.h): items holds the gathered slots alone
// (feat [n_items][items.slots.n]); code [n_items][dd.n] and dict_feat in device memory.
struct DictTable {
  ItemTable items;
  CatalogItemSlots all;     // every slot, the gathered ones first: S_c
  CatalogItemSlots dslots;  // the dictionary slots alone: their U
  CatalogDicts dd;
  const int32_t *code, *dict_feat;
};

// What both kinds of launches start with, on arrays in device memory: base and U of the requests, padded to `rows`
// (whole tiles of the launches that follow).  cap: the longest context, in [1, max_row_nnz].  items: U towards every
// slot's field, one block behind the other, instead of towards g.
static int catalog_prepare(ffm_engine *e, int32_t n_req, const int32_t *ctx_ptr, const int32_t *ctx_field, const int32_t *ctx_feat,
                           const float *ctx_val, int32_t ctx_nnz, int cap, int32_t g, const ItemTable *items, int rows, CatalogDev *out_cd) {
  const ModelDev &m = e->m;
  const int lp = catalog_lp(m.lat_fmt, m.row_len) * (items ? items->slots.n : 1);
  int rc;
  if ((rc = e->grow(&e->cat.base, &e->cat_base_cap, static_cast<size_t>(rows)))) return rc;
  if ((rc = e->grow(&e->cat.shift, &e->cat_shift_cap, static_cast<size_t>(rows)))) return rc;
  if ((rc = e->grow(&e->cat_u, &e->cat_u_cap, static_cast<size_t>(rows) * lp * 4))) return rc;  // (fp32, or two planes of halves)
  CatalogDev cd = e->cat;
  cd.u = e->cat_u;
  cd.rows = rows;
  cd.lp = lp;
  // base_r: the bits of predict_batch on the context rows
  launch_row_kernel(e, Rows{n_req, ctx_nnz, ctx_ptr, ctx_field, ctx_feat, ctx_val, nullptr}, cap, false, cd.base, 0);
  const int lds_cap = std::min(cap, kPredLdsCap);
  if (items)
    LAUNCH(e, K_CATALOG_ITEMS_U, catalog_items_u_fn(m.lat_fmt), cdiv(rows, kPredRows), 64 * kPredRows, cand_ctx_lds_bytes(lds_cap), m, n_req,
           ctx_ptr, ctx_field, ctx_feat, ctx_val, items->slots, cd, cap, lds_cap);
  else
    LAUNCH(e, K_CATALOG_U, catalog_u_fn(m.lat_fmt), cdiv(rows, kPredRows), 64 * kPredRows, cand_ctx_lds_bytes(lds_cap), m, n_req, ctx_ptr,
           ctx_field, ctx_feat, ctx_val, g, cd, cap, lds_cap);
  *out_cd = cd;
  return FFM_OK;
}

// S_c of every item of the table into e->item_s, ahead of the launches that read it.
static int catalog_items_self(ffm_engine *e, const ItemTable &items) {
  if (int rc = e->grow(&e->item_s, &e->item_s_cap, static_cast<size_t>(items.n_items))) return rc;
  const int grid = static_cast<int>((static_cast<int64_t>(items.n_items) * 4 + 255) / 256);
  LAUNCH(e, K_CATALOG_ITEMS_SELF, catalog_items_self_fn(e->m.lat_fmt), grid, 256, 0, e->m, items.slots, items.feat,
         static_cast<int64_t>(items.n_items), e->item_s);
  return FFM_OK;
}

// What the item source takes behind the kernels' common arguments (cd.lp: U's whole row, slots.n blocks of Lp).
static CatalogItemSrc::Args catalog_items_args(const ffm_engine *e, const ItemTable &items, const CatalogDev &cd) {
  const int es = e->m.lat_fmt == SERVE_F16 ? 2 : 4;
  return CatalogItemSrc::Args{items.feat, e->m.n_feats, items.slots.n, cd.lp / items.slots.n * es / kCatChunkBytes};
}

// ---- dictionary slots (include/ffm_engine.h "Scoring a catalogue: dictionary slots"; kernels_catalog_dict.h) ---------

// S_c of every item of a table with dictionary slots into e->item_s.
static int catalog_dict_self(ffm_engine *e, const DictTable &t) {
  if (int rc = e->grow(&e->item_s, &e->item_s_cap, static_cast<size_t>(t.items.n_items))) return rc;
  const int grid = static_cast<int>((static_cast<int64_t>(t.items.n_items) * 4 + 255) / 256);
  LAUNCH(e, K_CATALOG_DICT_SELF, catalog_dict_self_fn(e->m.lat_fmt), grid, 256, 0, e->m, t.all, t.items.slots.n, t.items.feat, t.code, t.dd,
         t.dict_feat, static_cast<int64_t>(t.items.n_items), e->item_s);
  return FFM_OK;
}

// U of the dictionary slots and the partial scores P of every dictionary entry against the `rows` padded requests
// (the rows of the launches that follow: whole tiles), into e->dict_p [t.dd.col[t.dd.n]][rows].
static int catalog_dict_partials(ffm_engine *e, int32_t n_req, const int32_t *ctx_ptr, const int32_t *ctx_field, const int32_t *ctx_feat,
                                 const float *ctx_val, int cap, const DictTable &t, int rows) {
  const ModelDev &m = e->m;
  const int lp = catalog_lp(m.lat_fmt, m.row_len), nd = t.dd.n, cols = t.dd.col[nd];
  int rc;
  if ((rc = e->grow(&e->dict_u, &e->dict_u_cap, static_cast<size_t>(nd) * rows * lp * 4))) return rc;
  if ((rc = e->grow(&e->dict_shift, &e->dict_shift_cap, static_cast<size_t>(nd) * rows))) return rc;
  if ((rc = e->grow(&e->dict_p, &e->dict_p_cap, std::max<size_t>(1, static_cast<size_t>(cols) * rows)))) return rc;
  if (cols == 0) return FFM_OK;  // (empty dictionaries: every code is erased, and P is never read)
  const CatalogDev cd0{nullptr, e->dict_u, e->dict_shift, rows, lp};
  const int lds_cap = std::min(cap, kPredLdsCap);
  LAUNCH(e, K_CATALOG_DICT_U, catalog_dict_u_fn(m.lat_fmt), cdiv(rows * nd, kPredRows), 64 * kPredRows, cand_ctx_lds_bytes(lds_cap), m, n_req,
         ctx_ptr, ctx_field, ctx_feat, ctx_val, t.dslots, cd0, cap, lds_cap);
  for (int r0 = 0; r0 < rows;) {
    const int rt = catalog_dict_rt((rows - r0) / kCatTile);
    LAUNCH(e, K_CATALOG_DICT, catalog_dict_fn(m.lat_fmt, rt), cdiv(cols, kCatCands), 64 * kCatWaves, 0, reinterpret_cast<const char *>(m.lat),
           m.row_len, cd0, r0, t.dd, t.dict_feat, m.n_feats, e->dict_p);
    r0 += kCatTile * rt;
  }
  return FFM_OK;
}

// What the dictionary source takes behind the kernels' common arguments; cd: the gathered slots' (catalog_prepare).
static CatalogDictSrc::Args catalog_dict_args(const ffm_engine *e, const DictTable &t, const CatalogDev &cd) {
  return CatalogDictSrc::Args{catalog_items_args(e, t.items, cd), t.code, e->dict_p, t.dd, cd.rows};
}

// items: the columns are its n_cand items (g, first and v unused, first == 0), else the range's candidates.  dict: the
// items' table has dictionary slots (items == &dict->items then).
static int catalog_launch(ffm_engine *e, int32_t n_req, const int32_t *ctx_ptr, const int32_t *ctx_field, const int32_t *ctx_feat,
                          const float *ctx_val, int32_t ctx_nnz, int cap, int32_t g, int32_t first, int32_t n_cand, float v,
                          const ItemTable *items, const DictTable *dict, int32_t output_prob, float *out) {
  const ModelDev &m = e->m;
  const int L = m.row_len, es = m.lat_fmt == SERVE_F16 ? 2 : 4;
  CatalogDev cd;
  if (int rc = dict ? catalog_dict_self(e, *dict) : items ? catalog_items_self(e, *items) : FFM_OK) return rc;
  if (int rc = catalog_prepare(e, n_req, ctx_ptr, ctx_field, ctx_feat, ctx_val, ctx_nnz, cap, g, items, catalog_rows(n_req), &cd)) return rc;
  if (int rc = dict ? catalog_dict_partials(e, n_req, ctx_ptr, ctx_field, ctx_feat, ctx_val, cap, *dict, cd.rows) : FFM_OK) return rc;
  const char *const tab = reinterpret_cast<const char *>(m.lat) + static_cast<int64_t>(first) * L * es;
  const int grid = static_cast<int>((static_cast<int64_t>(n_cand) + kCatCands - 1) / kCatCands);
  for (int r0 = 0; r0 < n_req; r0 += 128) {
    const int rt = catalog_rt(cdiv(std::min(128, n_req - r0), kCatTile));
    if (dict)
      LAUNCH(e, K_CATALOG_DICT_GEMM, catalog_gemm_fn<CatalogDictSrc>(m.lat_fmt, rt), grid, 64 * kCatWaves, 0, tab,
             static_cast<const float *>(e->item_s), L, cd, r0, n_req, static_cast<int64_t>(n_cand), 1.0f, output_prob, out,
             catalog_dict_args(e, *dict, cd));
    else if (items)
      LAUNCH(e, K_CATALOG_ITEMS_GEMM, catalog_gemm_fn<CatalogItemSrc>(m.lat_fmt, rt), grid, 64 * kCatWaves, 0, tab,
             static_cast<const float *>(e->item_s), L, cd, r0, n_req, static_cast<int64_t>(n_cand), 1.0f, output_prob, out,
             catalog_items_args(e, *items, cd));
    else
      LAUNCH(e, K_CATALOG_GEMM, catalog_gemm_fn(m.lat_fmt, rt), grid, 64 * kCatWaves, 0, tab, static_cast<const float *>(m.lin_w + first), L, cd,
             r0, n_req, static_cast<int64_t>(n_cand), v, output_prob, out, CatalogSlabSrc::Args{});
  }
  HIP_TRY(hipGetLastError());
  return FFM_OK;
}

// The host calls' contexts into the engine's staging arrays (d_ctx_*), checked on the caller's thread before anything
// is queued.  *ctx_nnz: their entries; *cap: the longest context, at most max_row_nnz.
static int catalog_stage_contexts(ffm_engine *e, int32_t n_req, const int32_t *ctx_ptr, const int32_t *ctx_field, const int32_t *ctx_feat,
                                  const float *ctx_val, int32_t *out_nnz, int *out_cap) {
  int rc;
  if (!ctx_ptr) return fail(FFM_E_INVALID, "null array");
  if ((rc = cand_check_ptr(ctx_ptr, n_req, "ctx_ptr"))) return rc;
  const int32_t ctx_nnz = ctx_ptr[n_req];
  if (ctx_nnz > 0 && (!ctx_field || !ctx_feat)) return fail(FFM_E_INVALID, "null field / feat array");
  int longest = 1;  // (a context beyond max_row_nnz is the row kernel's to flag: NaN for its request, FFM_E_CAPACITY from the call)
  for (int32_t r = 0; r < n_req; r++) longest = std::max(longest, ctx_ptr[r + 1] - ctx_ptr[r]);
  const size_t n_ptr = static_cast<size_t>(n_req) + 1, n_ctx = std::max<size_t>(1, static_cast<size_t>(ctx_nnz));
  if ((rc = e->grow(&e->d_ctx_ptr, &e->ctx_ptr_cap, n_ptr))) return rc;
  if ((rc = e->grow(&e->d_ctx_field, &e->ctx_field_cap, n_ctx))) return rc;
  if ((rc = e->grow(&e->d_ctx_feat, &e->ctx_feat_cap, n_ctx))) return rc;
  if ((rc = e->grow(&e->d_ctx_val, &e->ctx_val_cap, n_ctx))) return rc;
  // ---- copies, the values nobody sent, hashed ids: behind one another on the engine's stream, as score_candidates
  hipStream_t st = e->stream;
  HIP_TRY(hipMemcpyAsync(e->d_ctx_ptr, ctx_ptr, sizeof(int32_t) * n_ptr, hipMemcpyHostToDevice, st));
  if (ctx_nnz > 0) {
    HIP_TRY(hipMemcpyAsync(e->d_ctx_field, ctx_field, sizeof(int32_t) * ctx_nnz, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(e->d_ctx_feat, ctx_feat, sizeof(int32_t) * ctx_nnz, hipMemcpyHostToDevice, st));
    if (ctx_val) HIP_TRY(hipMemcpyAsync(e->d_ctx_val, ctx_val, sizeof(float) * ctx_nnz, hipMemcpyHostToDevice, st));
    else
      hipLaunchKernelGGL(fill_ones_kernel, dim3(std::max(1, std::min(256, cdiv(cdiv(ctx_nnz, 4), 256)))), dim3(256), 0, st,
                         e->d_ctx_val, static_cast<unsigned>(ctx_nnz));
    if (e->hash_ids) launch_hash_ids(e, st, ctx_nnz, e->d_ctx_field, e->d_ctx_feat, e->d_ctx_feat, e->d_ctx_val);
  }
  *out_nnz = ctx_nnz;
  *out_cap = std::min(longest, e->max_row_nnz);
  return FFM_OK;
}

int ffm_engine_score_catalog_device(ffm_engine *e, int32_t n_req, const int32_t *ctx_ptr, const int32_t *ctx_field,
                                    const int32_t *ctx_feat, const float *ctx_val, int32_t cand_field, int32_t cand_first,
                                    int32_t n_cand, float cand_val, int32_t ctx_nnz, int32_t ctx_cap, int32_t output_prob,
                                    float *out) {
  if (int rc = catalog_check(e, n_req, cand_field, cand_first, n_cand)) return rc;
  if (int rc = catalog_matrix_check(n_req, n_cand)) return rc;
  if (int rc = catalog_ready(e)) return rc;
  if (n_req == 0 || n_cand == 0) return FFM_OK;
  if (ctx_nnz < 0 || ctx_cap < 0) return fail(FFM_E_INVALID, "negative ctx_nnz / ctx_cap");
  if (!ctx_ptr || !out || (ctx_nnz > 0 && (!ctx_field || !ctx_feat || !ctx_val))) return fail(FFM_E_INVALID, "null array");
  // (a context beyond the engine's row limit is flagged by the row kernel whatever the cap says)
  const int cap = std::max(1, std::min(ctx_cap, e->max_row_nnz));
  return catalog_launch(e, n_req, ctx_ptr, ctx_field, ctx_feat, ctx_val, ctx_nnz, cap, cand_field, cand_first, n_cand, cand_val,
                        nullptr, nullptr, output_prob, out);
}

int ffm_engine_score_catalog(ffm_engine *e, int32_t n_req, const int32_t *ctx_ptr, const int32_t *ctx_field, const int32_t *ctx_feat,
                             const float *ctx_val, int32_t cand_field, int32_t cand_first, int32_t n_cand, float cand_val,
                             int32_t output_prob, float *out) {
  int rc = catalog_check(e, n_req, cand_field, cand_first, n_cand);
  if (rc || (rc = catalog_matrix_check(n_req, n_cand)) || (rc = catalog_ready(e))) return rc;
  if (n_req == 0 || n_cand == 0) return FFM_OK;
  if (!out) return fail(FFM_E_INVALID, "null array");
  const size_t n_out = static_cast<size_t>(n_req) * n_cand;
  int32_t ctx_nnz = 0;
  int cap = 1;
  if ((rc = e->grow(&e->cat_out, &e->cat_out_cap, n_out))) return rc;  // (before anything is queued)
  if ((rc = catalog_stage_contexts(e, n_req, ctx_ptr, ctx_field, ctx_feat, ctx_val, &ctx_nnz, &cap))) return rc;
  rc = catalog_launch(e, n_req, e->d_ctx_ptr, e->d_ctx_field, e->d_ctx_feat, e->d_ctx_val, ctx_nnz, cap, cand_field, cand_first, n_cand,
                      cand_val, nullptr, nullptr, output_prob, e->cat_out);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(out, e->cat_out, sizeof(float) * n_out, hipMemcpyDeviceToHost, e->stream));
  return check_device_errors(e);
}

// ---- the best K (include/ffm_engine.h "Scoring a catalogue: the best K") -------------------------------------------

static int catalog_topk_check(ffm_engine *e, int32_t n_req, int32_t cand_field, int32_t cand_first, int32_t n_cand, int32_t top_k) {
  if (int rc = catalog_check(e, n_req, cand_field, cand_first, n_cand)) return rc;
  if (top_k < 1 || top_k > kTopkMax)
    return fail(FFM_E_INVALID, "top_k " + std::to_string(top_k) + " lies outside [1, " + std::to_string(kTopkMax) + "]");
  return catalog_ready(e);
}

// Request tiles of the launch that starts at request r0: what top_k allows, no more than are left.
static int catalog_topk_tiles(int n_req, int r0, int top_k) {
  return std::min(catalog_topk_rt(top_k), catalog_rt(cdiv(n_req - r0, kCatTile)));
}

// The requests of a top-K call in whole tiles of its launches.
static int catalog_topk_rows(int n_req, int top_k) {
  int rows = 0;
  while (rows < n_req) rows += kCatTile * catalog_topk_tiles(n_req, rows, top_k);
  return rows;
}

// The launches, on arrays in device memory; out_score / out_id [n_req][top_k] there too.  n_req > 0.  items, dict: as
// catalog_launch.
static int catalog_topk_launch(ffm_engine *e, int32_t n_req, const int32_t *ctx_ptr, const int32_t *ctx_field, const int32_t *ctx_feat,
                               const float *ctx_val, int32_t ctx_nnz, int cap, int32_t g, int32_t first, int32_t n_cand, float v,
                               const ItemTable *items, const DictTable *dict, int32_t top_k, int32_t output_prob, float *out_score,
                               int32_t *out_id) {
  const ModelDev &m = e->m;
  const int kp = catalog_topk_kp(top_k);
  if (n_cand == 0) {  // nothing to rank: the fill alone
    LAUNCH(e, K_CATALOG_TOPK_MERGE, catalog_topk_merge_kernel, n_req, kTopkMergeThreads, 0, static_cast<const unsigned long long *>(nullptr),
           static_cast<int64_t>(0), kp, top_k, static_cast<const float *>(nullptr), first, output_prob, out_score, out_id);
    HIP_TRY(hipGetLastError());
    return FFM_OK;
  }
  const int L = m.row_len, es = m.lat_fmt == SERVE_F16 ? 2 : 4;
  const int rows = catalog_topk_rows(n_req, top_k);
  const int64_t slabs = (static_cast<int64_t>(n_cand) + kCatCands - 1) / kCatCands;
  const int grid = static_cast<int>(std::min<int64_t>(slabs, e->grid_catalog > 0 ? e->grid_catalog : 2 * e->cu_count));
  const int64_t P = static_cast<int64_t>(grid) * kCatWaves;
  int rc;
  if ((rc = e->grow(&e->topk_part, &e->topk_part_cap, static_cast<size_t>(n_req) * P * kp))) return rc;
  CatalogDev cd;
  if ((rc = dict ? catalog_dict_self(e, *dict) : items ? catalog_items_self(e, *items) : FFM_OK)) return rc;
  if ((rc = catalog_prepare(e, n_req, ctx_ptr, ctx_field, ctx_feat, ctx_val, ctx_nnz, cap, g, items, rows, &cd))) return rc;
  if (dict && (rc = catalog_dict_partials(e, n_req, ctx_ptr, ctx_field, ctx_feat, ctx_val, cap, *dict, rows))) return rc;
  const char *const tab = reinterpret_cast<const char *>(m.lat) + static_cast<int64_t>(first) * L * es;
  for (int r0 = 0; r0 < n_req;) {
    const int rt = catalog_topk_tiles(n_req, r0, top_k);
    if (dict)
      LAUNCH(e, K_CATALOG_DICT_TOPK, catalog_topk_fn<CatalogDictSrc>(m.lat_fmt, rt), grid, 64 * kCatWaves, catalog_topk_lds_bytes(rt, kp), tab,
             static_cast<const float *>(e->item_s), L, cd, r0, n_req, static_cast<int64_t>(n_cand), 1.0f, top_k, kp, e->topk_part,
             catalog_dict_args(e, *dict, cd));
    else if (items)
      LAUNCH(e, K_CATALOG_ITEMS_TOPK, catalog_topk_fn<CatalogItemSrc>(m.lat_fmt, rt), grid, 64 * kCatWaves, catalog_topk_lds_bytes(rt, kp), tab,
             static_cast<const float *>(e->item_s), L, cd, r0, n_req, static_cast<int64_t>(n_cand), 1.0f, top_k, kp, e->topk_part,
             catalog_items_args(e, *items, cd));
    else
      LAUNCH(e, K_CATALOG_TOPK, catalog_topk_fn(m.lat_fmt, rt), grid, 64 * kCatWaves, catalog_topk_lds_bytes(rt, kp), tab,
             static_cast<const float *>(m.lin_w + first), L, cd, r0, n_req, static_cast<int64_t>(n_cand), v, top_k, kp, e->topk_part,
             CatalogSlabSrc::Args{});
    r0 += kCatTile * rt;
  }
  LAUNCH(e, K_CATALOG_TOPK_MERGE, catalog_topk_merge_kernel, n_req, kTopkMergeThreads, 0, static_cast<const unsigned long long *>(e->topk_part),
         P, kp, top_k, static_cast<const float *>(cd.base), first, output_prob, out_score, out_id);
  HIP_TRY(hipGetLastError());
  return FFM_OK;
}

int ffm_engine_score_catalog_topk_device(ffm_engine *e, int32_t n_req, const int32_t *ctx_ptr, const int32_t *ctx_field,
                                         const int32_t *ctx_feat, const float *ctx_val, int32_t cand_field, int32_t cand_first,
                                         int32_t n_cand, float cand_val, int32_t top_k, int32_t ctx_nnz, int32_t ctx_cap,
                                         int32_t output_prob, float *out_score, int32_t *out_id) {
  if (int rc = catalog_topk_check(e, n_req, cand_field, cand_first, n_cand, top_k)) return rc;
  if (n_req == 0) return FFM_OK;
  if (ctx_nnz < 0 || ctx_cap < 0) return fail(FFM_E_INVALID, "negative ctx_nnz / ctx_cap");
  if (!out_score || !out_id || (n_cand > 0 && (!ctx_ptr || (ctx_nnz > 0 && (!ctx_field || !ctx_feat || !ctx_val)))))
    return fail(FFM_E_INVALID, "null array");
  const int cap = std::max(1, std::min(ctx_cap, e->max_row_nnz));
  return catalog_topk_launch(e, n_req, ctx_ptr, ctx_field, ctx_feat, ctx_val, ctx_nnz, cap, cand_field, cand_first, n_cand, cand_val,
                             nullptr, nullptr, top_k, output_prob, out_score, out_id);
}

int ffm_engine_score_catalog_topk(ffm_engine *e, int32_t n_req, const int32_t *ctx_ptr, const int32_t *ctx_field,
                                  const int32_t *ctx_feat, const float *ctx_val, int32_t cand_field, int32_t cand_first,
                                  int32_t n_cand, float cand_val, int32_t top_k, int32_t output_prob, float *out_score,
                                  int32_t *out_id) {
  int rc = catalog_topk_check(e, n_req, cand_field, cand_first, n_cand, top_k);
  if (rc) return rc;
  if (n_req == 0) return FFM_OK;
  if (!out_score || !out_id) return fail(FFM_E_INVALID, "null array");
  const size_t n_out = static_cast<size_t>(n_req) * top_k;
  if ((rc = e->grow(&e->topk_score, &e->topk_score_cap, n_out)) || (rc = e->grow(&e->topk_id, &e->topk_id_cap, n_out))) return rc;
  int32_t ctx_nnz = 0;
  int cap = 1;
  if (n_cand > 0 && (rc = catalog_stage_contexts(e, n_req, ctx_ptr, ctx_field, ctx_feat, ctx_val, &ctx_nnz, &cap))) return rc;
  rc = catalog_topk_launch(e, n_req, e->d_ctx_ptr, e->d_ctx_field, e->d_ctx_feat, e->d_ctx_val, ctx_nnz, cap, cand_field, cand_first,
                           n_cand, cand_val, nullptr, nullptr, top_k, output_prob, e->topk_score, e->topk_id);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(out_score, e->topk_score, sizeof(float) * n_out, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(out_id, e->topk_id, sizeof(int32_t) * n_out, hipMemcpyDeviceToHost, e->stream));
  return check_device_errors(e);
}

// ---- items of several entries (include/ffm_engine.h "Scoring a catalogue: items of several entries") ----------------

// catalog_check's checks for an item table, and the table's slots into *t (t->feat: item_feat as it came).  No range
// check of ids: an id outside [0, n_feats) is an erased slot.
static int items_check(ffm_engine *e, int32_t n_req, int32_t n_slots, const int32_t *item_field, const int32_t *item_feat,
                       const float *item_val, int32_t n_items, ItemTable *t, const char *what = "score_items") {
  if (int rc = catalog_engine_check(e, what)) return rc;
  if (n_req < 0 || n_items < 0) return fail(FFM_E_INVALID, "negative n_req / n_items");
  if (n_slots < 1 || n_slots > kItemSlots)
    return fail(FFM_E_INVALID, "item_field: n_slots " + std::to_string(n_slots) + " lies outside [1, " + std::to_string(kItemSlots) + "]");
  if (!item_field) return fail(FFM_E_INVALID, "null array (item_field)");
  *t = ItemTable{};
  for (int a = 0; a < n_slots; a++) {
    if (item_field[a] < 0 || item_field[a] >= e->m.n_fields)
      return fail(FFM_E_INVALID, "item_field[" + std::to_string(a) + "] = " + std::to_string(item_field[a]) + " lies outside [0, n_fields)");
    for (int b = 0; b < a; b++)
      if (item_field[b] == item_field[a])
        return fail(FFM_E_INVALID, "item_field names field " + std::to_string(item_field[a]) + " twice: an item has one entry per field");
    t->slots.field[a] = item_field[a];
    t->slots.val[a] = item_val ? item_val[a] : 1.0f;
  }
  t->slots.n = n_slots;
  t->feat = item_feat;
  t->n_items = n_items;
  if (n_req > e->max_rows) return fail(FFM_E_CAPACITY, "more requests than max_batch_rows");
  return FFM_OK;
}

// The host calls' item_feat into the engine's copy (t->feat: in host memory on entry, the copy afterwards), hashed
// under its slot's field on an engine with FFM_FLAG_HASH_IDS, behind one another on the engine's stream.
static int items_stage(ffm_engine *e, ItemTable *t) {
  const int m = t->slots.n;
  const size_t n = static_cast<size_t>(t->n_items) * m;
  int rc;
  if ((rc = e->grow(&e->d_item_feat, &e->item_feat_cap, n))) return rc;
  if (e->hash_ids && (rc = e->grow(&e->d_item_field, &e->item_field_cap, n))) return rc;
  hipStream_t st = e->stream;
  HIP_TRY(hipMemcpyAsync(e->d_item_feat, t->feat, sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
  if (e->hash_ids) {
    hipLaunchKernelGGL(catalog_items_fields_kernel, dim3(static_cast<unsigned>(std::min<size_t>(1024, (n + 255) / 256))), dim3(256), 0, st,
                       t->slots, static_cast<int64_t>(n), e->d_item_field);
    const size_t piece = static_cast<size_t>(m) << 27;  // whole items, and entries an int32 counts
    for (size_t at = 0; at < n; at += piece)
      launch_hash_ids(e, st, static_cast<int32_t>(std::min(piece, n - at)), e->d_item_field + at, e->d_item_feat + at, e->d_item_feat + at);
  }
  t->feat = e->d_item_feat;
  return FFM_OK;
}

int ffm_engine_score_items_device(ffm_engine *e, int32_t n_req, const int32_t *ctx_ptr, const int32_t *ctx_field, const int32_t *ctx_feat,
                                  const float *ctx_val, int32_t n_slots, const int32_t *item_field, const int32_t *item_feat,
                                  const float *item_val, int32_t n_items, int32_t ctx_nnz, int32_t ctx_cap, int32_t output_prob,
                                  float *out) {
  ItemTable t;
  if (int rc = items_check(e, n_req, n_slots, item_field, item_feat, item_val, n_items, &t)) return rc;
  if (int rc = catalog_matrix_check(n_req, n_items)) return rc;
  if (int rc = catalog_ready(e)) return rc;
  if (n_req == 0 || n_items == 0) return FFM_OK;
  if (ctx_nnz < 0 || ctx_cap < 0) return fail(FFM_E_INVALID, "negative ctx_nnz / ctx_cap");
  if (!ctx_ptr || !out || !item_feat || (ctx_nnz > 0 && (!ctx_field || !ctx_feat || !ctx_val))) return fail(FFM_E_INVALID, "null array");
  const int cap = std::max(1, std::min(ctx_cap, e->max_row_nnz));
  return catalog_launch(e, n_req, ctx_ptr, ctx_field, ctx_feat, ctx_val, ctx_nnz, cap, 0, 0, n_items, 1.0f, &t, nullptr, output_prob, out);
}

int ffm_engine_score_items(ffm_engine *e, int32_t n_req, const int32_t *ctx_ptr, const int32_t *ctx_field, const int32_t *ctx_feat,
                           const float *ctx_val, int32_t n_slots, const int32_t *item_field, const int32_t *item_feat,
                           const float *item_val, int32_t n_items, int32_t output_prob, float *out) {
  ItemTable t;
  int rc = items_check(e, n_req, n_slots, item_field, item_feat, item_val, n_items, &t);
  if (rc || (rc = catalog_matrix_check(n_req, n_items)) || (rc = catalog_ready(e))) return rc;
  if (n_req == 0 || n_items == 0) return FFM_OK;
  if (!out || !item_feat) return fail(FFM_E_INVALID, "null array");
  const size_t n_out = static_cast<size_t>(n_req) * n_items;
  int32_t ctx_nnz = 0;
  int cap = 1;
  if ((rc = e->grow(&e->cat_out, &e->cat_out_cap, n_out))) return rc;  // (before anything is queued)
  if ((rc = catalog_stage_contexts(e, n_req, ctx_ptr, ctx_field, ctx_feat, ctx_val, &ctx_nnz, &cap)) || (rc = items_stage(e, &t))) return rc;
  rc = catalog_launch(e, n_req, e->d_ctx_ptr, e->d_ctx_field, e->d_ctx_feat, e->d_ctx_val, ctx_nnz, cap, 0, 0, n_items, 1.0f, &t, nullptr, output_prob,
                      e->cat_out);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(out, e->cat_out, sizeof(float) * n_out, hipMemcpyDeviceToHost, e->stream));
  return check_device_errors(e);
}

static int items_topk_check(ffm_engine *e, int32_t n_req, int32_t n_slots, const int32_t *item_field, const int32_t *item_feat,
                            const float *item_val, int32_t n_items, int32_t top_k, ItemTable *t) {
  if (int rc = items_check(e, n_req, n_slots, item_field, item_feat, item_val, n_items, t)) return rc;
  if (top_k < 1 || top_k > kTopkMax)
    return fail(FFM_E_INVALID, "top_k " + std::to_string(top_k) + " lies outside [1, " + std::to_string(kTopkMax) + "]");
  return catalog_ready(e);
}

int ffm_engine_score_items_topk_device(ffm_engine *e, int32_t n_req, const int32_t *ctx_ptr, const int32_t *ctx_field,
                                       const int32_t *ctx_feat, const float *ctx_val, int32_t n_slots, const int32_t *item_field,
                                       const int32_t *item_feat, const float *item_val, int32_t n_items, int32_t top_k, int32_t ctx_nnz,
                                       int32_t ctx_cap, int32_t output_prob, float *out_score, int32_t *out_id) {
  ItemTable t;
  if (int rc = items_topk_check(e, n_req, n_slots, item_field, item_feat, item_val, n_items, top_k, &t)) return rc;
  if (n_req == 0) return FFM_OK;
  if (ctx_nnz < 0 || ctx_cap < 0) return fail(FFM_E_INVALID, "negative ctx_nnz / ctx_cap");
  if (!out_score || !out_id || (n_items > 0 && (!ctx_ptr || !item_feat || (ctx_nnz > 0 && (!ctx_field || !ctx_feat || !ctx_val)))))
    return fail(FFM_E_INVALID, "null array");
  const int cap = std::max(1, std::min(ctx_cap, e->max_row_nnz));
  return catalog_topk_launch(e, n_req, ctx_ptr, ctx_field, ctx_feat, ctx_val, ctx_nnz, cap, 0, 0, n_items, 1.0f, &t, nullptr, top_k, output_prob,
                             out_score, out_id);
}

int ffm_engine_score_items_topk(ffm_engine *e, int32_t n_req, const int32_t *ctx_ptr, const int32_t *ctx_field, const int32_t *ctx_feat,
                                const float *ctx_val, int32_t n_slots, const int32_t *item_field, const int32_t *item_feat,
                                const float *item_val, int32_t n_items, int32_t top_k, int32_t output_prob, float *out_score,
                                int32_t *out_id) {
  ItemTable t;
  int rc = items_topk_check(e, n_req, n_slots, item_field, item_feat, item_val, n_items, top_k, &t);
  if (rc) return rc;
  if (n_req == 0) return FFM_OK;
  if (!out_score || !out_id || (n_items > 0 && !item_feat)) return fail(FFM_E_INVALID, "null array");
  const size_t n_out = static_cast<size_t>(n_req) * top_k;
  if ((rc = e->grow(&e->topk_score, &e->topk_score_cap, n_out)) || (rc = e->grow(&e->topk_id, &e->topk_id_cap, n_out))) return rc;
  int32_t ctx_nnz = 0;
  int cap = 1;
  if (n_items > 0 && ((rc = catalog_stage_contexts(e, n_req, ctx_ptr, ctx_field, ctx_feat, ctx_val, &ctx_nnz, &cap)) || (rc = items_stage(e, &t))))
    return rc;
  rc = catalog_topk_launch(e, n_req, e->d_ctx_ptr, e->d_ctx_field, e->d_ctx_feat, e->d_ctx_val, ctx_nnz, cap, 0, 0, n_items, 1.0f, &t, nullptr, top_k,
                           output_prob, e->topk_score, e->topk_id);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(out_score, e->topk_score, sizeof(float) * n_out, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(out_id, e->topk_id, sizeof(int32_t) * n_out, hipMemcpyDeviceToHost, e->stream));
  return check_device_errors(e);
}

// ---- dictionary slots: the entry points (include/ffm_engine.h "Scoring a catalogue: dictionary slots") ---------------

// items_check's checks over all n_gather + n_dict slots, the counts and dict_ptr, and the table into *t (t->items.feat,
// t->code, t->dict_feat: the arrays as they came).  top_k: 0 for the matrix calls (it decides the padded requests, and
// with them the size of P).
static int dict_check(ffm_engine *e, int32_t n_req, int32_t n_gather, int32_t n_dict, const int32_t *item_field, const int32_t *item_feat,
                      const int32_t *item_code, const int32_t *dict_ptr, const int32_t *dict_feat, const float *item_val, int32_t n_items,
                      int32_t top_k, DictTable *t) {
  if (int rc = catalog_engine_check(e, "score_items_dict")) return rc;
  if (n_gather < 1) return fail(FFM_E_INVALID, "n_gather " + std::to_string(n_gather) + " lies below 1: ffm_engine_score_catalog scores a lone dictionary");
  if (n_dict < 1) return fail(FFM_E_INVALID, "n_dict " + std::to_string(n_dict) + " lies below 1: ffm_engine_score_items scores a table without dictionaries");
  ItemTable all;
  const int32_t n_slots = static_cast<int32_t>(std::min<int64_t>(static_cast<int64_t>(n_gather) + n_dict, kItemSlots + 1));
  if (int rc = items_check(e, n_req, n_slots, item_field, item_feat, item_val, n_items, &all)) return rc;
  if (!dict_ptr) return fail(FFM_E_INVALID, "null array (dict_ptr)");
  if (int rc = cand_check_ptr(dict_ptr, n_dict, "dict_ptr")) return rc;
  *t = DictTable{};
  t->all = all.slots;
  t->items = all;
  t->items.slots.n = n_gather;
  t->dslots.n = t->dd.n = n_dict;
  int64_t cols = 0;
  for (int a = 0; a <= n_dict; a++) {
    t->dd.ptr[a] = dict_ptr[a];
    t->dd.col[a] = static_cast<int>(std::min<int64_t>(cols, 2147483647ll));
    if (a == n_dict) break;
    t->dslots.field[a] = all.slots.field[n_gather + a];
    t->dslots.val[a] = all.slots.val[n_gather + a];
    cols += (static_cast<int64_t>(dict_ptr[a + 1]) - dict_ptr[a] + 31) / 32 * 32;
  }
  t->code = item_code;
  t->dict_feat = dict_feat;
  const int rows = top_k > 0 ? catalog_topk_rows(n_req, std::min(top_k, kTopkMax)) : catalog_rows(n_req);
  if (cols * std::max(rows, 1) > 2147483647ll)
    return fail(FFM_E_CAPACITY, "the padded requests times the dictionaries' padded entries exceed 2^31 - 1 partial scores: split the requests");
  return FFM_OK;
}

// The host calls' item_feat, item_code and dict_feat into the engine's copies (t's three arrays: in host memory on entry,
// the copies afterwards), behind one another on the engine's stream; on an engine with FFM_FLAG_HASH_IDS item_feat is
// hashed under its slots' fields (items_stage) and dict_feat under each dictionary's field.
static int dict_stage(ffm_engine *e, DictTable *t) {
  int rc;
  if ((rc = items_stage(e, &t->items))) return rc;
  const size_t n_code = static_cast<size_t>(t->items.n_items) * t->dd.n, n_ids = static_cast<size_t>(t->dd.ptr[t->dd.n]);
  if ((rc = e->grow(&e->d_item_code, &e->item_code_cap, std::max<size_t>(1, n_code)))) return rc;
  if ((rc = e->grow(&e->d_dict_feat, &e->dict_feat_cap, std::max<size_t>(1, n_ids)))) return rc;
  if (e->hash_ids && (rc = e->grow(&e->d_dict_field, &e->dict_field_cap, std::max<size_t>(1, n_ids)))) return rc;
  hipStream_t st = e->stream;
  HIP_TRY(hipMemcpyAsync(e->d_item_code, t->code, sizeof(int32_t) * n_code, hipMemcpyHostToDevice, st));
  if (n_ids > 0) {
    HIP_TRY(hipMemcpyAsync(e->d_dict_feat, t->dict_feat, sizeof(int32_t) * n_ids, hipMemcpyHostToDevice, st));
    if (e->hash_ids) {  // under each dictionary's field; codes are positions, never hashed
      hipLaunchKernelGGL(catalog_dict_fields_kernel, dim3(static_cast<unsigned>(std::min<size_t>(1024, (n_ids + 255) / 256))), dim3(256), 0, st,
                         t->dslots, t->dd, static_cast<int>(n_ids), e->d_dict_field);
      launch_hash_ids(e, st, static_cast<int32_t>(n_ids), e->d_dict_field, e->d_dict_feat, e->d_dict_feat);
    }
  }
  t->code = e->d_item_code;
  t->dict_feat = e->d_dict_feat;
  return FFM_OK;
}

// (dict_feat may be null when every dictionary is empty)
static bool dict_arrays_null(const DictTable &t) { return !t.items.feat || !t.code || (t.dd.ptr[t.dd.n] > 0 && !t.dict_feat); }

int ffm_engine_score_items_dict_device(ffm_engine *e, int32_t n_req, const int32_t *ctx_ptr, const int32_t *ctx_field,
                                       const int32_t *ctx_feat, const float *ctx_val, int32_t n_gather, int32_t n_dict,
                                       const int32_t *item_field, const int32_t *item_feat, const int32_t *item_code,
                                       const int32_t *dict_ptr, const int32_t *dict_feat, const float *item_val, int32_t n_items,
                                       int32_t ctx_nnz, int32_t ctx_cap, int32_t output_prob, float *out) {
  DictTable t;
  if (int rc = dict_check(e, n_req, n_gather, n_dict, item_field, item_feat, item_code, dict_ptr, dict_feat, item_val, n_items, 0, &t)) return rc;
  if (int rc = catalog_matrix_check(n_req, n_items)) return rc;
  if (int rc = catalog_ready(e)) return rc;
  if (n_req == 0 || n_items == 0) return FFM_OK;
  if (ctx_nnz < 0 || ctx_cap < 0) return fail(FFM_E_INVALID, "negative ctx_nnz / ctx_cap");
  if (!ctx_ptr || !out || dict_arrays_null(t) || (ctx_nnz > 0 && (!ctx_field || !ctx_feat || !ctx_val))) return fail(FFM_E_INVALID, "null array");
  const int cap = std::max(1, std::min(ctx_cap, e->max_row_nnz));
  return catalog_launch(e, n_req, ctx_ptr, ctx_field, ctx_feat, ctx_val, ctx_nnz, cap, 0, 0, n_items, 1.0f, &t.items, &t, output_prob, out);
}

int ffm_engine_score_items_dict(ffm_engine *e, int32_t n_req, const int32_t *ctx_ptr, const int32_t *ctx_field, const int32_t *ctx_feat,
                                const float *ctx_val, int32_t n_gather, int32_t n_dict, const int32_t *item_field,
                                const int32_t *item_feat, const int32_t *item_code, const int32_t *dict_ptr, const int32_t *dict_feat,
                                const float *item_val, int32_t n_items, int32_t output_prob, float *out) {
  DictTable t;
  int rc = dict_check(e, n_req, n_gather, n_dict, item_field, item_feat, item_code, dict_ptr, dict_feat, item_val, n_items, 0, &t);
  if (rc || (rc = catalog_matrix_check(n_req, n_items)) || (rc = catalog_ready(e))) return rc;
  if (n_req == 0 || n_items == 0) return FFM_OK;
  if (!out || dict_arrays_null(t)) return fail(FFM_E_INVALID, "null array");
  const size_t n_out = static_cast<size_t>(n_req) * n_items;
  int32_t ctx_nnz = 0;
  int cap = 1;
  if ((rc = e->grow(&e->cat_out, &e->cat_out_cap, n_out))) return rc;  // (before anything is queued)
  if ((rc = catalog_stage_contexts(e, n_req, ctx_ptr, ctx_field, ctx_feat, ctx_val, &ctx_nnz, &cap)) || (rc = dict_stage(e, &t))) return rc;
  rc = catalog_launch(e, n_req, e->d_ctx_ptr, e->d_ctx_field, e->d_ctx_feat, e->d_ctx_val, ctx_nnz, cap, 0, 0, n_items, 1.0f, &t.items, &t,
                      output_prob, e->cat_out);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(out, e->cat_out, sizeof(float) * n_out, hipMemcpyDeviceToHost, e->stream));
  return check_device_errors(e);
}

static int dict_topk_check(ffm_engine *e, int32_t n_req, int32_t n_gather, int32_t n_dict, const int32_t *item_field,
                           const int32_t *item_feat, const int32_t *item_code, const int32_t *dict_ptr, const int32_t *dict_feat,
                           const float *item_val, int32_t n_items, int32_t top_k, DictTable *t) {
  if (int rc = dict_check(e, n_req, n_gather, n_dict, item_field, item_feat, item_code, dict_ptr, dict_feat, item_val, n_items,
                          std::max(top_k, 1), t))
    return rc;
  if (top_k < 1 || top_k > kTopkMax)
    return fail(FFM_E_INVALID, "top_k " + std::to_string(top_k) + " lies outside [1, " + std::to_string(kTopkMax) + "]");
  return catalog_ready(e);
}

int ffm_engine_score_items_dict_topk_device(ffm_engine *e, int32_t n_req, const int32_t *ctx_ptr, const int32_t *ctx_field,
                                            const int32_t *ctx_feat, const float *ctx_val, int32_t n_gather, int32_t n_dict,
                                            const int32_t *item_field, const int32_t *item_feat, const int32_t *item_code,
                                            const int32_t *dict_ptr, const int32_t *dict_feat, const float *item_val, int32_t n_items,
                                            int32_t top_k, int32_t ctx_nnz, int32_t ctx_cap, int32_t output_prob, float *out_score,
                                            int32_t *out_id) {
  DictTable t;
  if (int rc = dict_topk_check(e, n_req, n_gather, n_dict, item_field, item_feat, item_code, dict_ptr, dict_feat, item_val, n_items, top_k, &t))
    return rc;
  if (n_req == 0) return FFM_OK;
  if (ctx_nnz < 0 || ctx_cap < 0) return fail(FFM_E_INVALID, "negative ctx_nnz / ctx_cap");
  if (!out_score || !out_id || (n_items > 0 && (!ctx_ptr || dict_arrays_null(t) || (ctx_nnz > 0 && (!ctx_field || !ctx_feat || !ctx_val)))))
    return fail(FFM_E_INVALID, "null array");
  const int cap = std::max(1, std::min(ctx_cap, e->max_row_nnz));
  return catalog_topk_launch(e, n_req, ctx_ptr, ctx_field, ctx_feat, ctx_val, ctx_nnz, cap, 0, 0, n_items, 1.0f, &t.items, &t, top_k,
                             output_prob, out_score, out_id);
}

int ffm_engine_score_items_dict_topk(ffm_engine *e, int32_t n_req, const int32_t *ctx_ptr, const int32_t *ctx_field,
                                     const int32_t *ctx_feat, const float *ctx_val, int32_t n_gather, int32_t n_dict,
                                     const int32_t *item_field, const int32_t *item_feat, const int32_t *item_code,
                                     const int32_t *dict_ptr, const int32_t *dict_feat, const float *item_val, int32_t n_items,
                                     int32_t top_k, int32_t output_prob, float *out_score, int32_t *out_id) {
  DictTable t;
  int rc = dict_topk_check(e, n_req, n_gather, n_dict, item_field, item_feat, item_code, dict_ptr, dict_feat, item_val, n_items, top_k, &t);
  if (rc) return rc;
  if (n_req == 0) return FFM_OK;
  if (!out_score || !out_id || (n_items > 0 && dict_arrays_null(t))) return fail(FFM_E_INVALID, "null array");
  const size_t n_out = static_cast<size_t>(n_req) * top_k;
  if ((rc = e->grow(&e->topk_score, &e->topk_score_cap, n_out)) || (rc = e->grow(&e->topk_id, &e->topk_id_cap, n_out))) return rc;
  int32_t ctx_nnz = 0;
  int cap = 1;
  if (n_items > 0 && ((rc = catalog_stage_contexts(e, n_req, ctx_ptr, ctx_field, ctx_feat, ctx_val, &ctx_nnz, &cap)) || (rc = dict_stage(e, &t))))
    return rc;
  rc = catalog_topk_launch(e, n_req, e->d_ctx_ptr, e->d_ctx_field, e->d_ctx_feat, e->d_ctx_val, ctx_nnz, cap, 0, 0, n_items, 1.0f, &t.items, &t,
                           top_k, output_prob, e->topk_score, e->topk_id);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(out_score, e->topk_score, sizeof(float) * n_out, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(out_id, e->topk_id, sizeof(int32_t) * n_out, hipMemcpyDeviceToHost, e->stream));
  return check_device_errors(e);
}

// ---- per-request item lists (include/ffm_engine.h "Scoring a catalogue: per-request item lists"; kernels_catalog_lists.h)

// items_check under the call's own name, and what the lists' kernel asks of the shape.
static int lists_check(ffm_engine *e, int32_t n_req, int32_t n_slots, const int32_t *item_field, const int32_t *item_feat,
                       const float *item_val, int32_t n_items, ItemTable *t) {
  if (int rc = items_check(e, n_req, n_slots, item_field, item_feat, item_val, n_items, t, "score_item_lists")) return rc;
  if (catalog_lists_lu(e->m.row_len) > kListMaxLu)
    return fail(FFM_E_UNSUPPORTED, "score_item_lists stages a block of U in LDS: n_fields * n_factors above " + std::to_string(kListMaxLu) +
                                       " is not supported");
  return catalog_ready(e);
}

// The workgroups of catalog_lists_kernel for lists of up to list_cap entries.
static int lists_grid_check(int32_t n_req, int32_t list_cap) {
  if (static_cast<int64_t>(n_req) * cdiv(list_cap, kListSeg) > (1ll << 23))
    return fail(FFM_E_CAPACITY, "n_req times the longest list exceeds 2^30 list positions: split the call");
  return FFM_OK;
}

// The launches, on arrays in device memory: base, U as plain floats, S of the n_list entries, the dot products.
// n_req, n_list, list_cap > 0; cap: the longest context, in [1, max_row_nnz].
static int catalog_lists_launch(ffm_engine *e, int32_t n_req, const int32_t *ctx_ptr, const int32_t *ctx_field, const int32_t *ctx_feat,
                                const float *ctx_val, int32_t ctx_nnz, int cap, const ItemTable &t, const int32_t *list_ptr,
                                const int32_t *list_item, int32_t n_list, int32_t list_cap, int32_t output_prob, float *out) {
  const ModelDev &m = e->m;
  const int lu = catalog_lists_lu(m.row_len), n_slots = t.slots.n;
  int rc;
  if ((rc = e->grow(&e->cat.base, &e->cat_base_cap, static_cast<size_t>(n_req)))) return rc;
  if ((rc = e->grow(&e->cat_u, &e->cat_u_cap, static_cast<size_t>(n_req) * n_slots * lu * sizeof(float)))) return rc;
  if ((rc = e->grow(&e->list_s, &e->list_s_cap, static_cast<size_t>(n_list)))) return rc;
  float *const u = reinterpret_cast<float *>(e->cat_u);
  // base_r: the bits of predict_batch on the context rows (as catalog_prepare)
  launch_row_kernel(e, Rows{n_req, ctx_nnz, ctx_ptr, ctx_field, ctx_feat, ctx_val, nullptr}, cap, false, e->cat.base, 0);
  const int lds_cap = std::min(cap, kPredLdsCap);
  const int parts = cdiv(n_slots * lu, kListURun);  // (at most 512 a request: the grid stays far inside 2^31)
  LAUNCH(e, K_CATALOG_LISTS_U, catalog_lists_u_fn(m.lat_fmt), cdiv(n_req * parts, kPredRows), 64 * kPredRows, cand_ctx_lds_bytes(lds_cap), m,
         n_req, ctx_ptr, ctx_field, ctx_feat, ctx_val, t.slots, u, lu, parts, cap, lds_cap);
  const int grid_s = static_cast<int>((static_cast<int64_t>(n_list) * 4 + 255) / 256);
  LAUNCH(e, K_CATALOG_LISTS_SELF, catalog_lists_self_fn(m.lat_fmt), grid_s, 256, 0, m, t.slots, t.feat, t.n_items, list_item,
         static_cast<int64_t>(n_list), e->list_s);
  LAUNCH(e, K_CATALOG_LISTS, catalog_lists_fn(m.lat_fmt), dim3(n_req, cdiv(list_cap, kListSeg)), 256, 2 * lu * sizeof(float),
         reinterpret_cast<const char *>(m.lat), m.row_len, m.n_feats, n_slots, t.feat, t.n_items, list_ptr, list_item,
         static_cast<int64_t>(n_list), list_cap, static_cast<const float *>(u), lu, static_cast<const float *>(e->list_s),
         static_cast<const float *>(e->cat.base), output_prob, out);
  HIP_TRY(hipGetLastError());
  return FFM_OK;
}

int ffm_engine_score_item_lists_device(ffm_engine *e, int32_t n_req, const int32_t *ctx_ptr, const int32_t *ctx_field,
                                       const int32_t *ctx_feat, const float *ctx_val, int32_t n_slots, const int32_t *item_field,
                                       const int32_t *item_feat, const float *item_val, int32_t n_items, const int32_t *list_ptr,
                                       const int32_t *list_item, int32_t ctx_nnz, int32_t ctx_cap, int32_t n_list, int32_t list_cap,
                                       int32_t output_prob, float *out) {
  ItemTable t;
  if (int rc = lists_check(e, n_req, n_slots, item_field, item_feat, item_val, n_items, &t)) return rc;
  if (ctx_nnz < 0 || ctx_cap < 0 || n_list < 0 || list_cap < 0) return fail(FFM_E_INVALID, "negative ctx_nnz / ctx_cap / n_list / list_cap");
  if (n_req == 0 || n_list == 0 || list_cap == 0) return FFM_OK;
  if (int rc = lists_grid_check(n_req, list_cap)) return rc;
  if (!ctx_ptr || !out || !list_ptr || !list_item || (n_items > 0 && !item_feat) || (ctx_nnz > 0 && (!ctx_field || !ctx_feat || !ctx_val)))
    return fail(FFM_E_INVALID, "null array");
  const int cap = std::max(1, std::min(ctx_cap, e->max_row_nnz));
  return catalog_lists_launch(e, n_req, ctx_ptr, ctx_field, ctx_feat, ctx_val, ctx_nnz, cap, t, list_ptr, list_item, n_list, list_cap,
                              output_prob, out);
}

int ffm_engine_score_item_lists(ffm_engine *e, int32_t n_req, const int32_t *ctx_ptr, const int32_t *ctx_field, const int32_t *ctx_feat,
                                const float *ctx_val, int32_t n_slots, const int32_t *item_field, const int32_t *item_feat,
                                const float *item_val, int32_t n_items, const int32_t *list_ptr, const int32_t *list_item,
                                int32_t output_prob, float *out) {
  ItemTable t;
  int rc = lists_check(e, n_req, n_slots, item_field, item_feat, item_val, n_items, &t);
  if (rc) return rc;
  if (n_req == 0) return FFM_OK;
  if (!list_ptr) return fail(FFM_E_INVALID, "null array (list_ptr)");
  if ((rc = cand_check_ptr(list_ptr, n_req, "list_ptr"))) return rc;
  const int32_t n_list = list_ptr[n_req];
  if (n_list == 0) return FFM_OK;
  if (!out || !list_item || (n_items > 0 && !item_feat)) return fail(FFM_E_INVALID, "null array");
  int32_t list_cap = 0;
  for (int32_t r = 0; r < n_req; r++) list_cap = std::max(list_cap, list_ptr[r + 1] - list_ptr[r]);
  if ((rc = lists_grid_check(n_req, list_cap))) return rc;
  int32_t ctx_nnz = 0;
  int cap = 1;
  if ((rc = e->grow(&e->list_out, &e->list_out_cap, static_cast<size_t>(n_list))) ||  // (before anything is queued)
      (rc = e->grow(&e->d_list_ptr, &e->list_ptr_cap, static_cast<size_t>(n_req) + 1)) ||
      (rc = e->grow(&e->d_list_item, &e->list_item_cap, static_cast<size_t>(n_list))))
    return rc;
  if ((rc = catalog_stage_contexts(e, n_req, ctx_ptr, ctx_field, ctx_feat, ctx_val, &ctx_nnz, &cap))) return rc;
  if (n_items > 0 && (rc = items_stage(e, &t))) return rc;
  HIP_TRY(hipMemcpyAsync(e->d_list_ptr, list_ptr, sizeof(int32_t) * (static_cast<size_t>(n_req) + 1), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->d_list_item, list_item, sizeof(int32_t) * n_list, hipMemcpyHostToDevice, e->stream));
  rc = catalog_lists_launch(e, n_req, e->d_ctx_ptr, e->d_ctx_field, e->d_ctx_feat, e->d_ctx_val, ctx_nnz, cap, t, e->d_list_ptr, e->d_list_item,
                            n_list, list_cap, output_prob, e->list_out);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(out, e->list_out, sizeof(float) * n_list, hipMemcpyDeviceToHost, e->stream));
  return check_device_errors(e);
}
