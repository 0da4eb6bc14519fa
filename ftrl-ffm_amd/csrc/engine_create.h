// engine_create.h -- ffm_engine_create as a sequence of steps, each returning an FFM_* code: the argument checks,
// the FFM_* switches (read_switches: the only place of this file that asks the environment), the model's
// geometry, streams, the model arrays, the scratch all sets share and then every set's own, the grouping's
// sort, the two fast-math proofs, the dynamic-LDS opt-in, the initial weights.  A half-built engine is owned by
// a guard whose deleter is ffm_engine_destroy, so every step leaves with a plain return.
// Part of engine.hip's translation unit (included inside its extern "C" block).

static int hash_ids_check(int32_t model_type, int32_t n_feats, int32_t n_fields, const int32_t *field_start);  // (engine_hash.h)
static int serve_create_check(const ffm_engine_config *cfg);  // (engine_serve.h)
static int norm_ready(ffm_engine *e);  // (engine_norm.h)

// What the environment sets.  An empty optional: the switch is not set, and the default -- an ffm_engine member's
// initializer, or what a later step works out for the shape -- stands.
struct Switches {
  bool hash_ids = false;  // FFM_ENGINE_HASH_IDS=1: FFM_FLAG_HASH_IDS on whatever the caller's flags say (every rank of a group)
  int metrics = 0;        // FFM_ENGINE_METRICS=<mask>: channels on from the start (rank 0 of a group keeps them)
  char row_refresh = 0;   // FFM_ENGINE_ROW_REFRESH: its first character ('0' .. '3')
  std::optional<bool> serial, super_wait, prep_after_row, pull_after_row, eval_defer_off, predict_waves, few_stage, own_sort;
  std::optional<int> update_split, update_order, wide_max_nnz, grid_pull, grid_push, grid_hot, grid_small, grid_walk, grid_giant, grid_norm;
  std::optional<int> row_threads, row_park, row_park_budget, row_hold, super_min;
  std::optional<int> range_sort;  // FFM_RANGE_SORT: 0 off, 1 on, more: that many equal ranges
};
extern "C++" {
template <typename T, typename U>
static void take(T &dst, const std::optional<U> &v) { if (v) dst = static_cast<T>(*v); }
// null: a combination no launch uses (engine_select.h) -- nothing to opt in
template <typename Fn>
static int lds_opt_in(Fn *kernel, size_t bytes) {
  if (kernel) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes)));
  return FFM_OK;
}
// A host vector into a device array of the engine's.
template <typename T>
static int upload(ffm_engine *e, const std::vector<T> &host, T **dev) {
  if (int rc = e->alloc(dev, host.size())) return rc;
  HIP_TRY(hipMemcpy(*dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
  return FFM_OK;
}
}

static Switches read_switches() {
  Switches sw;
  if (const char *sv = std::getenv("FFM_ENGINE_HASH_IDS")) sw.hash_ids = sv[0] == '1';
  if (const char *sv = std::getenv("FFM_ENGINE_METRICS")) sw.metrics = std::atoi(sv) & 3;
  if (const char *sv = std::getenv("FFM_ENGINE_ROW_REFRESH")) sw.row_refresh = sv[0];
  if (const char *sv = std::getenv("FFM_ENGINE_SERIAL")) sw.serial = sv[0] == '1';
  if (const char *sv = std::getenv("FFM_UPDATE_SPLIT")) sw.update_split = std::atoi(sv);
  if (const char *sv = std::getenv("FFM_UPDATE_ORDER")) {
    // a permutation of the digits {0, 1, 2} (first range last) or nothing: any other value would run
    // one range of the update launch twice and drop another
    const int o = std::atoi(sv);
    const int d0 = o % 10, d1 = o / 10 % 10, d2 = o / 100;
    if (o >= 0 && d2 <= 2 && d0 <= 2 && d1 <= 2 && d0 != d1 && d0 != d2 && d1 != d2) sw.update_order = o;
  }
  if (const char *sv = std::getenv("FFM_SUPER_WAIT")) sw.super_wait = sv[0] != '0';
  if (const char *sv = std::getenv("FFM_PREP_AFTER_ROW")) sw.prep_after_row = sv[0] == '1';
  if (const char *sv = std::getenv("FFM_PULL_AFTER_ROW")) sw.pull_after_row = sv[0] == '1';
  if (const char *sv = std::getenv("FFM_EVAL_DEFER")) sw.eval_defer_off = sv[0] == '0';
  if (const char *sv = std::getenv("FFM_PREDICT_WAVE")) sw.predict_waves = std::atoi(sv) != 0;
  if (const char *sv = std::getenv("FFM_WIDE_NNZ")) sw.wide_max_nnz = std::atoi(sv);
  if (const char *sv = std::getenv("FFM_GRID_PULL")) sw.grid_pull = std::max(1, std::atoi(sv));
  if (const char *sv = std::getenv("FFM_GRID_PUSH")) sw.grid_push = std::min(24, std::max(1, std::atoi(sv)));
  if (const char *sv = std::getenv("FFM_GRID_NORM")) sw.grid_norm = std::max(1, std::atoi(sv));
  if (const char *sv = std::getenv("FFM_GRID_HOT")) sw.grid_hot = std::max(1, std::atoi(sv));
  if (const char *sv = std::getenv("FFM_GRID_SMALL")) sw.grid_small = std::max(1, std::atoi(sv));
  if (const char *sv = std::getenv("FFM_GRID_WALK")) sw.grid_walk = std::max(1, std::atoi(sv));
  if (const char *sv = std::getenv("FFM_GRID_GIANT")) sw.grid_giant = std::max(1, std::atoi(sv));
  if (const char *sv = std::getenv("FFM_ROW_THREADS")) sw.row_threads = std::max(64, std::min(kRowMaxThreads, std::atoi(sv) / 64 * 64));
  if (const char *sv = std::getenv("FFM_ROW_PARK")) sw.row_park = std::atoi(sv);
  if (const char *sv = std::getenv("FFM_ROW_PARK_BUDGET")) sw.row_park_budget = std::atoi(sv);
  if (const char *sv = std::getenv("FFM_ROW_HOLD")) sw.row_hold = std::max(0, std::atoi(sv));
  if (const char *sv = std::getenv("FFM_SUPER_MIN")) sw.super_min = std::max(kGiantMin, std::atoi(sv));
  if (const char *sv = std::getenv("FFM_FEW_STAGE")) sw.few_stage = sv[0] != '0';
  if (const char *sv = std::getenv("FFM_OWN_SORT")) sw.own_sort = std::atoi(sv) != 0;
  if (const char *sv = std::getenv("FFM_RANGE_SORT")) sw.range_sort = std::atoi(sv);
  return sw;
}

// Everything that can be refused without a device, and then the device itself.
static int check_config(const ffm_engine_config *cfg, bool hash_ids) {
  if (cfg->model_type < FFM_MODEL_LR || cfg->model_type > FFM_MODEL_FFM)
    return fail(FFM_E_INVALID, "invalid model_type, expect LR(0), FM(1) or FFM(2)");
  if (cfg->n_feats <= 0) return fail(FFM_E_INVALID, "n_feats must be positive");
  if (cfg->model_type == FFM_MODEL_FFM && cfg->n_fields <= 0)
    return fail(FFM_E_INVALID, "n_fields must be positive for FFM");
  if (cfg->model_type != FFM_MODEL_LR && cfg->n_factors <= 0)
    return fail(FFM_E_INVALID, "n_factors must be positive for FM/FFM");
  if (cfg->model_type == FFM_MODEL_FM && cfg->n_factors > kTermsCap)
    return fail(FFM_E_UNSUPPORTED, "FM n_factors above 2048 is not supported");
  if (cfg->max_batch_rows <= 0 || cfg->max_batch_nnz <= 0)
    return fail(FFM_E_INVALID, "max_batch_rows / max_batch_nnz must be positive");
  if (cfg->n_shards < 1 || cfg->shard_rank < 0 || cfg->shard_rank >= cfg->n_shards)
    return fail(FFM_E_INVALID, "invalid n_shards / shard_rank");
  if (cfg->n_shards > 1 && cfg->model_type != FFM_MODEL_FFM)
    return fail(FFM_E_UNSUPPORTED, "field-pair sharding applies to FFM only");
  if (cfg->n_shards > 1 && cfg->n_fields > 64)
    return fail(FFM_E_UNSUPPORTED, "field-pair sharding supports up to 64 fields");
  // FFM_FLAG_NORM_ROWS (engine_norm.h): a row's length is a sum over ALL of its entries
  if ((cfg->flags & FFM_FLAG_NORM_ROWS) && cfg->n_shards > 1)
    return fail(FFM_E_INVALID, "FFM_FLAG_NORM_ROWS needs a whole model (n_shards == 1): a shard does not own whole rows");
  // FFM_FLAG_SERVE_F32 / _F16: a serving engine (engine_serve.h) -- its shape is checked like the arguments above
  if (cfg->flags & (FFM_FLAG_SERVE_F32 | FFM_FLAG_SERVE_F16))
    if (int rc_s = serve_create_check(cfg)) return rc_s;
  // (an argument error like the ones above: reported whether or not there is a device)
  if (hash_ids)
    if (int rc_h = hash_ids_check(cfg->model_type, cfg->n_feats, cfg->n_fields, cfg->field_start)) return rc_h;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
    return fail(FFM_E_DEVICE, "no HIP device available (this library has no CPU fallback)");
  if (cfg->device_id < 0 || cfg->device_id >= n_dev)
    return fail(FFM_E_INVALID, "device_id out of range");
  HIP_TRY(hipSetDevice(cfg->device_id));
  return FFM_OK;
}

// The engine's members that a switch or the shape sets (no device call).
static void apply_switches(ffm_engine *e, const Switches &sw) {
  const ffm_engine_config *cfg = &e->cfg;
  take(e->serial, sw.serial);
  take(e->update_split, sw.update_split);
  take(e->update_order, sw.update_order);
  take(e->super_wait, sw.super_wait);
  take(e->prep_after_row, sw.prep_after_row);
  take(e->eval_defer_off, sw.eval_defer_off);
  take(e->predict_waves, sw.predict_waves);
  take(e->wide_max_nnz, sw.wide_max_nnz);
  take(e->grid_pull, sw.grid_pull);
  take(e->grid_push, sw.grid_push);
  take(e->grid_norm, sw.grid_norm);
  take(e->grid_hot, sw.grid_hot);
  take(e->grid_small, sw.grid_small);
  take(e->grid_walk, sw.grid_walk);
  take(e->grid_giant, sw.grid_giant);
  // (a sharded rank's row holds 1/n_shards of the pairs and facts, walked directly; 64-thread row
  // workgroups measured the same as 256)
  // a shard's row holds ~1/n_shards of the pairs: one wave per row, so that (with the small LDS
  // footprint of short rows) many more rows are in flight per CU
  if (cfg->n_shards > 1) e->row_threads = 64;
  take(e->row_threads, sw.row_threads);
  take(e->row_park, sw.row_park);
  take(e->row_park_budget, sw.row_park_budget);
  take(e->row_hold, sw.row_hold);
  // (the lean once-only kernel of a compact shard holds six waves per SIMD: 1152 workgroups
  // measured 2.5 % per step better than 768 on an 8-GPU rank's blocks)
  if (cfg->n_shards > 1) e->grid_single = 1152;
  // (... and its flat few-occurrence kernel, 126 VGPRs = four waves per SIMD, fills the chip at 1024
  // workgroups: an emulated rank's step 1.615 -> 1.605 ms)
  if (cfg->n_shards > 1 && !sw.grid_small) e->grid_small = 1024;
  const char rr = sw.row_refresh;
  const int64_t per = cfg->n_factors % 4 == 0 ? static_cast<int64_t>(cfg->n_fields) * cfg->n_factors / 4
                                              : static_cast<int64_t>(cfg->n_fields) * cfg->n_factors;
  e->pre_refresh = cfg->model_type == FFM_MODEL_FFM && cfg->n_fields <= 64 &&
                   static_cast<int64_t>(e->max_nnz) * per < (1ll << 31) && rr != '1';
  if (rr == '0') e->refresh_mode = 1;
  if (rr == '2') e->refresh_mode = 2;
  if (rr == '3') e->refresh_mode = 3;
}

// The model's geometry (ModelDev, except its device pointers) and, sharded, the field-pair partition.
static int plan_model(ffm_engine *e, const Switches &sw, ShardPlan *plan) {
  const ffm_engine_config *cfg = &e->cfg;
  ModelDev &m = e->m;
  m.type = cfg->model_type;
  m.n_feats = cfg->n_feats;
  m.n_fields = cfg->model_type == FFM_MODEL_FFM ? cfg->n_fields : 1;
  m.n_factors = cfg->model_type == FFM_MODEL_LR ? 0 : cfg->n_factors;
  e->logical_len = cfg->model_type == FFM_MODEL_FFM ? cfg->n_fields * cfg->n_factors
                   : cfg->model_type == FFM_MODEL_FM ? cfg->n_factors : 0;
  m.n_shards = cfg->n_shards;
  m.shard_rank = cfg->shard_rank;
  m.bias_own = 1;
  m.huge_min = kHugeMin;
  m.giant_min = cfg->model_type == FFM_MODEL_FM ? kFmGiantMin : kGiantMin;
  m.range_len = cfg->model_type == FFM_MODEL_FM ? kFmRange : kRange;
  m.huge_min = std::min(m.huge_min, m.giant_min - 1);  // (the lists: big <= huge_min < huge < giant_min <= giant)
  m.super_min = kSuperMin;
  take(m.super_min, sw.super_min);
  m.few_stage = 1;
  take(m.few_stage, sw.few_stage);
  m.lat_fmt = (cfg->flags & FFM_FLAG_SERVE_F32 ? SERVE_F32 : 0) | (cfg->flags & FFM_FLAG_SERVE_F16 ? SERVE_F16 : 0);
  m.rec_slots = m.n_fields;
  e->n_records = cfg->n_feats;
  // field-pair partition: this shard's ranges, and (with per-field id ranges) compact storage
  const bool compact = cfg->n_shards > 1 && cfg->field_start != nullptr;
  if (cfg->field_start && cfg->model_type == FFM_MODEL_FFM) {
    e->field_start.assign(cfg->field_start, cfg->field_start + cfg->n_fields + 1);
    bool ok = e->field_start[0] == 0 && e->field_start[cfg->n_fields] == cfg->n_feats;
    for (int f = 0; f < cfg->n_fields; f++) ok = ok && e->field_start[f] <= e->field_start[f + 1];
    if (!ok) return fail(FFM_E_INVALID, "field_start must ascend from 0 to n_feats");
  }
  if (cfg->n_shards > 1) {
    *plan = make_shard_plan(cfg->n_fields, cfg->n_shards, compact);
    m.bias_own = plan->bias_owner == cfg->shard_rank ? 1 : 0;
    if (compact) {
      int widest = 1;
      for (int f = 0; f < cfg->n_fields; f++) widest = std::max(widest, plan->n(cfg->shard_rank, f));
      m.rec_slots = widest;
      e->n_records = 0;
      for (int f = 0; f < cfg->n_fields; f++)
        if (plan->n(cfg->shard_rank, f) > 0) e->n_records += e->field_start[f + 1] - e->field_start[f];
      if (e->n_records == 0) e->n_records = 1;
    }
  }
  m.row_len = cfg->model_type == FFM_MODEL_FFM ? m.rec_slots * cfg->n_factors
              : cfg->model_type == FFM_MODEL_FM ? cfg->n_factors : 0;
  m.h = Hyper{cfg->w_alpha, cfg->w_beta, cfg->w_l1, cfg->w_l2, 1.0f / cfg->w_alpha, 0,
              (cfg->flags & FFM_FLAG_LEARN) ? 1 : 0};
  if (static_cast<int64_t>(cfg->n_fields) * cfg->n_factors > (1 << 24))
    return fail(FFM_E_UNSUPPORTED, "n_fields*n_factors too large");
  if (static_cast<int64_t>(cfg->max_batch_nnz) / (kSmallMax + 1) * ((m.row_len + 7) / 8 + 1) >= (1ll << 31))
    return fail(FFM_E_UNSUPPORTED, "max_batch_nnz * row_len too large for 32-bit work-item ids");
  return FFM_OK;
}

// Streams: the runtime multiplexes them onto few hardware queues (ffm_engine: no more than stream + 2 side + prep).
static int create_streams(ffm_engine *e) {
  if (e->cfg.stream) {
    e->stream = static_cast<hipStream_t>(e->cfg.stream);
  } else {
    HIP_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    e->own_stream = true;
  }
  // (priority streams for the hot / very hot update: measured +45 % per step; for the look-ahead
  // grouping: the same)
  HIP_TRY(hipStreamCreateWithFlags(&e->aux3, hipStreamNonBlocking));
  HIP_TRY(hipStreamCreateWithFlags(&e->aux4, hipStreamNonBlocking));
  // The upload kernel runs on the prep queue, ahead of the block's grouping.  (Round 4 moved it, for
  // long steps, behind the update's chain kernel on that kernel's stream; the update is one launch on
  // the main stream now and that stream is otherwise empty: 1.060 ms there, 1.048 ms on the prep
  // queue.)
  HIP_TRY(hipStreamCreateWithFlags(&e->prep, hipStreamNonBlocking));
  for (hipEvent_t *ev : {&e->ev_fork, &e->ev_fork2, &e->ev_join, &e->ev_join2})
    HIP_TRY(hipEventCreateWithFlags(ev, hipEventDisableTiming));
  for (int i = 0; i < ffm_engine::kSets; i++) {
    HIP_TRY(hipEventCreateWithFlags(&e->ev_grouped[i], hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&e->ev_set_free[i], hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&e->ev_row_done[i], hipEventDisableTiming));
  }
  return FFM_OK;
}

// The model in HBM, zeroed, and the small tables ModelDev points to: which slots, linear terms and records
// this shard owns, the hashed ids' ranges.
static int alloc_model(ffm_engine *e, const ShardPlan &plan) {
  const ffm_engine_config *cfg = &e->cfg;
  ModelDev &m = e->m;
  int rc;
  const size_t nf = static_cast<size_t>(cfg->n_feats);
  // floats allocated for the latent part: records of (n, z, w), or a serving engine's table of w alone in
  // 4- or 2-byte elements (row_len is a multiple of 4 there) -- and then no (n, z) of the bias or the linear part
  const size_t n_w = static_cast<size_t>(e->n_records) * static_cast<size_t>(m.row_len);
  const size_t n_lat = m.lat_fmt == SERVE_F16 ? n_w / 2 : m.lat_fmt == SERVE_F32 ? n_w : 3 * n_w;
  const size_t n_bias = serving(e) ? 1 : 4;
  if ((rc = e->alloc(&m.bias3, n_bias))) return rc;
  HIP_TRY(hipMemsetAsync(m.bias3, 0, n_bias * sizeof(float), e->stream));
  for (float **lin : {&m.lin_n, &m.lin_z, &m.lin_w}) {
    if (serving(e) && lin != &m.lin_w) continue;
    if ((rc = e->alloc(lin, nf))) return rc;
    HIP_TRY(hipMemsetAsync(*lin, 0, nf * sizeof(float), e->stream));
  }
  if ((rc = e->alloc(&m.lat, n_lat))) return rc;
  if (n_lat) HIP_TRY(hipMemsetAsync(m.lat, 0, n_lat * sizeof(float), e->stream));
  if (m.type == FFM_MODEL_FFM && m.n_fields <= 64) {  // (the field masks of the scratch sets: alloc_set)
    std::vector<unsigned long long> own(m.n_fields, 0ull);
    for (int fa = 0; fa < m.n_fields; fa++)
      for (int fb = 0; fb < m.n_fields; fb++)
        if (m.n_shards <= 1 || plan.owns(m.shard_rank, fa, fb)) own[fa] |= 1ull << fb;
    if ((rc = upload(e, own, &e->d_ownmask))) return rc;
    m.ownmask = e->d_ownmask;
  }
  if (m.n_shards > 1) {
    // this shard's ranges (and, compact, the record index of every kept field) on the device
    const bool compact = cfg->field_start != nullptr;
    const int F = m.n_fields, r = m.shard_rank;
    std::vector<int> lo(F), cnt(F), lin(F);
    std::vector<long long> base(F, -1);
    long long next = 0;
    for (int f = 0; f < F; f++) {
      lo[f] = plan.lo(r, f);
      cnt[f] = plan.n(r, f);
      lin[f] = plan.lin_owner[f] == r ? 1 : 0;
      if (compact && cnt[f] > 0) { base[f] = next; next += e->field_start[f + 1] - e->field_start[f]; }
    }
    int *d_lo = nullptr, *d_n = nullptr, *d_lin = nullptr;
    if ((rc = upload(e, lo, &d_lo)) || (rc = upload(e, cnt, &d_n)) || (rc = upload(e, lin, &d_lin))) return rc;
    m.own_lo = d_lo;
    m.own_n = d_n;
    m.lin_own = d_lin;
    e->lin_any = std::any_of(lin.begin(), lin.end(), [](int v) { return v != 0; });
    if (compact) {
      int *d_fs = nullptr;
      long long *d_base = nullptr;
      if ((rc = upload(e, e->field_start, &d_fs)) || (rc = upload(e, base, &d_base))) return rc;
      m.field_start = d_fs;
      m.rec_base = d_base;
    }
  }
  if (e->hash_ids) {
    e->hm = ftrl_hash::Map{nullptr, cfg->n_feats, m.n_fields, m.type == FFM_MODEL_FFM ? 1 : 0};
    if (!e->field_start.empty()) {  // (kept for FFM only; widths checked above)
      if ((rc = upload(e, e->field_start, &e->d_hash_start))) return rc;
      e->hm.start = e->d_hash_start;
    }
  }
  return FFM_OK;
}

// What all scratch sets share -- `shared` is what every set starts from (alloc_set) --, the engine's own
// staging arrays, and the size of a set's sort workspace.  Shared is what the row kernel and the update write:
// one block's update ends before the next one's starts.  Everything the GROUPING writes is a set's own.
static int alloc_shared(ffm_engine *e, Scratch *shared) {
  const ffm_engine_config *cfg = &e->cfg;
  const ModelDev &m = e->m;
  Scratch &s = *shared;
  int rc;
  const size_t R = static_cast<size_t>(e->max_rows), E = static_cast<size_t>(e->max_nnz);
  // partial sums of the giant features' folds
  const size_t max_segs = E / kSeg + E / kFmGiantMin + 2, rl = static_cast<size_t>(std::max(1, m.row_len));
  const bool lat_model = cfg->model_type != FFM_MODEL_LR, ffm_m = cfg->model_type == FFM_MODEL_FFM;
  const size_t chunks = !ffm_m ? 1 : cfg->n_factors <= 64
                            ? (static_cast<size_t>(m.rec_slots) + 64 / cfg->n_factors - 1) / (64 / cfg->n_factors)
                            : static_cast<size_t>(m.rec_slots) * ((cfg->n_factors + 63) / 64);
  if ((rc = e->alloc(&s.segP, lat_model ? max_segs * rl : 1)) || (rc = e->alloc(&s.segG, lat_model ? max_segs * rl : 1)) ||
      (rc = e->alloc(&s.segD, ffm_m ? max_segs * rl : 1)) || (rc = e->alloc(&s.segF, ffm_m ? max_segs * chunks * 3 : 1)) ||
      (rc = e->alloc(&s.gcap, ffm_m ? (E / kGiantMin + 2) * rl : 1)))
    return rc;
  if ((rc = e->alloc(&e->d_err, 1))) return rc;
  HIP_TRY(hipMemsetAsync(e->d_err, 0, sizeof(int), e->stream));
  s.err = e->d_err;
  if ((rc = e->alloc(&s.head, R * static_cast<size_t>(m.n_fields))) || (rc = e->alloc(&s.next, E)) ||
      (rc = e->alloc(&s.rowtab, R * static_cast<size_t>(m.n_fields))) || (rc = e->alloc(&s.logit, R)) ||
      (rc = e->alloc(&s.tg, R)) || (rc = e->alloc(&s.loss, R)) ||
      (rc = e->alloc(&s.svx, R * static_cast<size_t>(m.type == FFM_MODEL_FM ? m.n_factors : 1))))
    return rc;
  // stable LSD radix sort of (feature id, entry) pairs: key bits = those of the sentinel n_feats
  e->sort_bits = 1;
  while (e->sort_bits < 32 && (static_cast<uint64_t>(cfg->n_feats) >> e->sort_bits) != 0) e->sort_bits++;
  unsigned *no_key = nullptr;  // (a size query: no array is read)
  int *no_occ = nullptr;
  HIP_TRY(rocprim::radix_sort_pairs<GroupSortConfig>(nullptr, e->sort_tmp_bytes, no_key, no_key,
                                    rocprim::counting_iterator<int>(0), no_occ, E, 0u, e->sort_bits, e->stream));
  e->sort_tmp_bytes = std::max(e->sort_tmp_bytes, sort_scratch_bytes(E));
  HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&e->h_super), sizeof(int) * ffm_engine::kSets, hipHostMallocMapped));
  std::memset(e->h_super, 0, sizeof(int) * ffm_engine::kSets);
  HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&s.n_super), e->h_super, 0));  // (set si's slot: + si)
  // The host skips the longest features' two extra launches when it reads 0 here -- which is only
  // safe if a device store to this mapping actually lands: prove it once, else the
  // launches are always made.
  hipLaunchKernelGGL(host_word_probe_kernel, dim3(1), dim3(64), 0, e->stream, s.n_super, ffm_engine::kSets);
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->super_flag_ok = true;
  for (int si = 0; si < ffm_engine::kSets; si++) e->super_flag_ok = e->super_flag_ok && e->h_super[si] == 0x5eed + si;
  std::memset(e->h_super, 0, sizeof(int) * ffm_engine::kSets);
  // staging for the host-buffer entry points, ids of a get_rows / set_rows chunk, dense staging for get / set
  if ((rc = e->alloc(&e->d_ids, static_cast<size_t>(ffm_engine::kIdsCap))) || (rc = e->alloc(&e->d_row_ptr, R + 1)) ||
      (rc = e->alloc(&e->d_field, E)) || (rc = e->alloc(&e->d_feat, E)) || (rc = e->alloc(&e->d_val, E)) ||
      (rc = e->alloc(&e->d_label, R)) || (rc = e->alloc(&e->d_out, R)) || (rc = e->alloc(&e->d_loss_sum, 2)) ||
      (rc = e->alloc(&e->d_loss_part, kLossParts + 1)))
    return rc;
  HIP_TRY(hipMemsetAsync(e->d_loss_part, 0, sizeof(double) * (kLossParts + 1), e->stream));
  e->stage_floats = 16 << 20;  // 64 MiB dense staging for get/set
  if (static_cast<int64_t>(e->logical_len) > e->stage_floats) e->stage_floats = e->logical_len;
  return e->alloc(&e->d_stage, static_cast<size_t>(e->stage_floats));
}

// (Not made here, and no scratch set's: the two ffm_engine::AblateSet, abl of field ablation and pabl of pair
// ablation -- scores, losses, loss sums with their partial sums and, on request, histograms for n_fields + 1 and
// n_fields (n_fields + 1) / 2 + 1 variants.  Each set is the engine's own, one per engine whatever kSets is: its
// calls are synchronous or ordered on the main stream, so no two blocks use it at once.  It is made by
// ffm_engine_ablation_enable / ffm_engine_pair_ablation_enable (engine_ablate.h: all of a call's arrays or none)
// through ffm_engine::alloc, so ffm_engine_destroy frees it with everything else; an engine that never enables
// either holds none of it.)
//
// Scratch set si: the one place that names a per-set array and its size.  The set starts as a copy of
// `shared` (alloc_shared), so a Scratch member that is named neither here nor there is null in every set.
static int alloc_set(ffm_engine *e, int si, const Scratch &shared) {
  const ModelDev &m = e->m;
  Scratch &t = e->sc[si];
  t = shared;
  t.n_super = shared.n_super + si;
  int rc;
  const size_t R = static_cast<size_t>(e->max_rows), E = static_cast<size_t>(e->max_nnz);
  if ((rc = e->alloc(&t.key, E)) || (rc = e->alloc(&t.skey, E)) || (rc = e->alloc(&t.row_of, E)) ||
      (rc = e->alloc(&t.occ, E)) || (rc = e->alloc(&t.occ2, E)) || (rc = e->alloc(&t.udesc, E)) ||
      (rc = e->alloc(&t.small, E)) || (rc = e->alloc(&t.few, E)) || (rc = e->alloc(&t.sdesc, E)) ||
      (rc = e->alloc(&t.big, E)) || (rc = e->alloc(&t.huge, E)) || (rc = e->alloc(&t.giant, E / kChainMin + 1)) ||
      (rc = e->alloc(&t.gseg, E / kChainMin + 1)) || (rc = e->alloc(&t.grange, E / kFmRange + E / kFmGiantMin + 2)) ||
      (rc = e->alloc(&t.counters, kNumCounters)) || (rc = e->alloc(&t.occpos, E)) || (rc = e->alloc(&t.uflag, E)))
    return rc;
  if (m.type == FFM_MODEL_FFM && m.n_fields <= 64)  // the field masks
    if ((rc = e->alloc(&t.rowmask, 2 * R)) || (rc = e->alloc(&t.gmask, E)) || (rc = e->alloc(&t.cmask, E))) return rc;
  unsigned char *tmp = nullptr;  // the sort's workspace (rocPRIM's, or kernels_sort.h's)
  if ((rc = e->alloc(&tmp, e->sort_tmp_bytes))) return rc;
  e->d_sort_tmp[si] = tmp;
  HIP_TRY(hipMemsetAsync(t.counters, 0, kNumCounters * sizeof(int), e->stream));
  return FFM_OK;
}

// Which sort the grouping uses depends on how long a step of this engine is (estimated from the
// largest block the engine was sized for).  Short steps wait for the look-ahead queue's chain of ~17
// launches one to one (FM k = 64: 0.32 ms per step of which 0.23 ms are its two kernels) and take the
// one-launch sort of kernels_sort.h (FM 0.323 -> 0.294 ms, FFM 8 x 16 at 4096 rows 0.139 -> 0.122); a
// long FFM step is saturated by its row kernel, a sort that actually runs beside it slows it (r05:
// 1.048 -> 1.094 ms), and the library sort's 1024-thread workgroups -- which only find room in the
// gaps -- are the better neighbour.  FFM 39 x 4 is the crossover (no difference).
static int choose_sort(ffm_engine *e, const Switches &sw) {
  const ffm_engine_config *cfg = &e->cfg;
  ModelDev &m = e->m;
  const double per_row = e->max_rows > 0 ? static_cast<double>(e->max_nnz) / e->max_rows : 0.0;
  const double phase_us = static_cast<double>(e->max_nnz) * std::max(0.0, per_row - 1.0) * m.n_factors / 0.44e6;
  const bool ffm4 = m.type == FFM_MODEL_FFM && m.n_factors % 4 == 0;
  e->own_sort = !(ffm4 && phase_us / std::max(1, m.n_shards) >= 100.0);  // (a shard does 1/n_shards of the pairs)
  take(e->own_sort, sw.own_sort);
  // The fields' id ranges are known (cfg->field_start): every range is sorted by a workgroup of its
  // own, one launch, no grid barrier (kernels_sort.h: group_sort_ranges_kernel).  FFM_RANGE_SORT=0/1
  // overrides; 1 without field_start cuts the id space into n_fields equal ranges (a block whose ids
  // crowd into one of them is still sorted correctly, by one workgroup).
  const bool have = !e->field_start.empty(), forced = sw.range_sort.has_value();
  // (by default only where a workgroup per range is quick: a whole model -- a compact shard's dropped
  // columns make every block irregular, so every workgroup would scan all keys twice -- and at most
  // 16 k entries per range -- a rank's 65 536-row blocks are 256 tiles per pass for ONE workgroup:
  // an emulated 8-GPU rank went 1.72 -> 2.25 ms per step with it)
  const bool quick = cfg->n_shards == 1 && static_cast<int64_t>(e->max_nnz) <= 16384ll * std::max(1, cfg->n_fields);
  const bool want = forced ? *sw.range_sort != 0 : (have && quick);
  if (want && (m.type == FFM_MODEL_FFM || forced)) {
    const int nr = have ? cfg->n_fields : (forced && *sw.range_sort > 1 ? std::min(1024, *sw.range_sort) : std::max(1, std::min(64, cfg->n_fields)));
    std::vector<int> st(static_cast<size_t>(nr) + 1);
    for (int f = 0; f <= nr; f++)
      st[f] = have ? e->field_start[f] : static_cast<int>(static_cast<int64_t>(cfg->n_feats) * f / nr);
    if (int rc = upload(e, st, &e->d_sort_start)) return rc;
    e->n_sort_ranges = nr;
    e->range_sort = true;
    // (the regular-block short cut needs range f to be field f's: only with the caller's field_start)
    if (have && m.type == FFM_MODEL_FFM) m.sort_start = e->d_sort_start;
    // ... and its look-ahead starts when the ROW kernel of the block enqueued last has ended, beside
    // that block's update launches (half of their wave slots are free, and they are not bound by
    // bandwidth) instead of at the block's end, beside the next block's saturated row kernel -- where
    // this sort, unlike the library's (whose 1024-thread workgroups wait for a CU to drain and so only
    // ever fill gaps), costs the row kernel 5 %: C5 driver shape 0.970 -> 0.949 ms, C3 0.531 -> 0.521
    // (profiles/r06_experiments.md).  FFM_PREP_AFTER_ROW=0/1 overrides.
    // (long steps only: a 4096 x 8 block's update phase is 70 us, shorter than the chain)
    if (!sw.prep_after_row) e->prep_after_row = !e->own_sort;
    // ... and from 4 M slot-factors per block on the block's upload waits for that event as well (C5: the
    // driver's 20-step shape 0.887-0.896 -> 0.877-0.884 ms, 200 steps 0.870 -> 0.868; C3, 1.2 M: 0.472 ->
    // 0.478, not taken).  FFM_PULL_AFTER_ROW=0/1 overrides.
    e->pull_after_row = e->prep_after_row && static_cast<int64_t>(e->max_nnz) * m.n_factors >= (1ll << 22);
    take(e->pull_after_row, sw.pull_after_row);
  }
  // the one-launch sort meets at a grid barrier: never more workgroups than the device holds of it,
  // and only on the architecture its hand-over of data between workgroups was validated on
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, cfg->device_id));
  int per_cu = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, group_sort_kernel, kSortThreads, 0));
  e->sort_grid_cap = std::max(1, per_cu * prop.multiProcessorCount);
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0 && std::strncmp(prop.gcnArchName, "gfx942", 6) != 0) e->own_sort = false;
  return FFM_OK;
}

// What a proof kernel left in the first counter of set 0; the counters are zeroed again behind it.
static int read_verdict(ffm_engine *e, int *bad) {
  int *counters = e->sc[0].counters;
  HIP_TRY(hipMemcpyAsync(bad, counters, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemsetAsync(counters, 0, kNumCounters * sizeof(int), e->stream));
  return FFM_OK;
}

// The two short sequences of ftrl_math.h, proven against the IEEE operations on this device before any
// kernel may use them.  Each proof kernel raises the first counter of set 0 on a mismatch.
static int prove_fast_math(ffm_engine *e) {
  const ffm_engine_config *cfg = &e->cfg;
  ModelDev &m = e->m;
  {
    // the five-instruction square root rests on this device's v_sqrt_f32 / v_rsq_f32: compare it
    // with sqrtf over its whole range (1.6e9 inputs, a few milliseconds) before any kernel uses it
    // (once per device and process: the answer is a property of the hardware)
    static std::atomic<int> verdict[64];  // 0 unknown, 1 exact, -1 differs
    const int dev = cfg->device_id & 63;
    int bad = verdict[dev].load() < 0 ? 1 : 0;
    if (verdict[dev].load() == 0) {
      hipLaunchKernelGGL(verify_sqrt_fast_kernel, dim3(16384), dim3(256), 0, e->stream, e->sc[0].counters);
      if (int rc = read_verdict(e, &bad)) return rc;
      verdict[dev].store(bad ? -1 : 1);
    }
    if (bad)
      return fail(FFM_E_UNSUPPORTED, "this device's v_sqrt_f32 / v_rsq_f32 do not give the correctly rounded "
                                     "square root in the short sequence the kernels use (built and proven for gfx950)");
  }
  if (cfg->w_alpha >= 0x1p-30f && cfg->w_alpha <= 0x1p30f) {
    // prove the short x/alpha sequence exact for this alpha before any kernel may use it
    int bad = 0;
    Hyper probe = m.h;
    probe.fast_div = 1;
    hipLaunchKernelGGL(verify_div_alpha_kernel, dim3(1u << 17), dim3(256), 0, e->stream, probe, e->sc[0].counters);
    if (int rc = read_verdict(e, &bad)) return rc;
    m.h.fast_div = bad ? 0 : 1;
    m.h.fast_w = m.h.fast_div && cfg->w_beta >= 0x1p-40f && cfg->w_beta <= 0x1p40f ? 1 : 0;
  }
  return FFM_OK;
}

// Dynamic LDS above the default limit must be asked for per kernel: every instantiation a launch can pick
// (engine_select.h) is opted in here, by walking the selectors' domains.
static int opt_in_lds(ffm_engine *e) {
  int rc;
  // the row kernels stage one row in dynamic LDS: opt in to what the longest admissible row needs
  const size_t lds = row_lds_bytes(e->max_row_nnz, e->m.n_fields, kTermsCap);
  if (lds > 150 * 1024) return fail(FFM_E_UNSUPPORTED, "max_row_nnz too large for the 160 KB of LDS per workgroup");
  const size_t park_budget = static_cast<size_t>(std::max(0, e->row_park_budget));
  if (lds > 32 * 1024 || park_budget > 32 * 1024) {
    const size_t bytes = std::max(lds, park_budget);
    for (int train = 0; train < 2; train++) {
      if ((rc = lds_opt_in(fm_row_fn(train), bytes))) return rc;
      for (int vec4 = 0; vec4 < 2; vec4++)
        for (int whole = 0; whole < 2; whole++)
          for (int hold = 0; hold <= 8; hold++)
            if ((rc = lds_opt_in(ffm_row_fn<>(train, vec4, whole, hold), bytes)) ||
                (rc = lds_opt_in(ffm_row_fn<const float *>(train, vec4, whole, hold), bytes)))
              return rc;
    }
  }
  // the FFM update launch: the tile pipelines' per-wave LDS regions of its (up to 16-wave) workgroups
  for (int nf = 1; nf <= 4; nf *= 2)
    for (int kinds = 1; kinds <= UPD_ALL; kinds++)
      for (int waves : {tile_waves(nf), kWideWaves})
        if ((rc = lds_opt_in(update_all_fn(nf, kinds, waves), tile_lds_bytes(nf, waves)))) return rc;
  return FFM_OK;
}

static int init_weights(ffm_engine *e) {
  const ffm_engine_config *cfg = &e->cfg;
  const bool skip = (cfg->flags & FFM_FLAG_SKIP_INIT) != 0;  // (the caller sets the state; the arrays are zeroed)
  if (!skip && serving(e))
    hipLaunchKernelGGL(serve_init_kernel, dim3(2048), dim3(256), 0, e->stream, e->m, cfg->init_mean, cfg->init_stddev, cfg->seed);
  else if (!skip)
    hipLaunchKernelGGL(init_weights_kernel, dim3(2048), dim3(256), 0, e->stream, e->m, e->logical_len,
                       cfg->init_mean, cfg->init_stddev, cfg->seed);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  return FFM_OK;
}

int ffm_engine_create(const ffm_engine_config *cfg, ffm_engine **out) {
  if (!cfg || !out) return fail(FFM_E_INVALID, "null config or output pointer");
  *out = nullptr;
  const Switches sw = read_switches();
  const bool hash_ids = (cfg->flags & FFM_FLAG_HASH_IDS) != 0 || sw.hash_ids;
  if (int rc_c = check_config(cfg, hash_ids)) return rc_c;
  // from here on every error leaves through the guard: ffm_engine_destroy copes with a half-built engine
  std::unique_ptr<ffm_engine, void (*)(ffm_engine *)> guard(new (std::nothrow) ffm_engine, ffm_engine_destroy);
  ffm_engine *e = guard.get();
  if (!e) return fail(FFM_E_NOMEM, "host allocation failed");
  e->cfg = *cfg;
  if (hash_ids) e->cfg.flags |= FFM_FLAG_HASH_IDS;
  e->hash_ids = hash_ids;
  e->max_rows = cfg->max_batch_rows;
  e->max_nnz = cfg->max_batch_nnz;
  if (cfg->max_row_nnz > 0) e->max_row_nnz = cfg->max_row_nnz;
  else if (cfg->flags & (FFM_FLAG_SERVE_F32 | FFM_FLAG_SERVE_F16)) e->max_row_nnz = kPredLdsCap;  // (a serving engine's rows are one wave's: no longer ones)
  apply_switches(e, sw);
  ShardPlan plan;
  Scratch shared{};
  int rc;
  if ((rc = plan_model(e, sw, &plan)) || (rc = create_streams(e)) || (rc = alloc_model(e, plan)) || (rc = alloc_shared(e, &shared)))
    return rc;
  for (int si = 0; si < ffm_engine::kSets; si++)
    if ((rc = alloc_set(e, si, shared))) return rc;
  e->norm_rows_on = (cfg->flags & FFM_FLAG_NORM_ROWS) != 0;
  if (e->norm_rows_on && (rc = norm_ready(e))) return rc;
  if ((rc = choose_sort(e, sw)) || (rc = prove_fast_math(e)) || (rc = opt_in_lds(e)) || (rc = init_weights(e))) return rc;
  if (sw.metrics && cfg->shard_rank == 0)
    if ((rc = ffm_engine_metrics_enable(e, sw.metrics))) return rc;
  *out = guard.release();
  return FFM_OK;
}
