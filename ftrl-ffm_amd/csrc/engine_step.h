// engine_step.h -- one block of rows on the device: grouping, look-ahead, forward, update, predict
// (the *_device entry points and the copying train_batch / predict_batch).
// Part of engine.hip's translation unit (included inside its extern "C" block).

// ---- one block of rows ---------------------------------------------------------------------

static int eval_launch_pending(ffm_engine *e);  // (engine_stage.h)
static void launch_metric(ffm_engine *e, int channel, int n_rows, const float *score, int is_prob, const int *label);  // (engine_metrics.h)
static void launch_keyed(ffm_engine *e, int channel, const Rows &rows, const float *score, int is_prob);  // (engine_keyed.h)
__global__ void loss_accumulate_kernel(double *acc, const double *one) { *acc += *one; }

// hold_eval: do not launch the deferred evaluation block now (predict_batch_async: it waits until this
// block's upload is submitted)
static int check_block(ffm_engine *e, int32_t n_rows, int32_t nnz, const void *row_ptr,
                       const void *field, const void *feat, const void *val, bool implicit_fields = false,
                       bool implicit_ones = false, bool hold_eval = false) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  // an evaluation block whose predict launch predict_batch_async deferred goes first (every entry
  // point that puts work on the main stream passes here)
  if (e->eval_pending.on && !hold_eval)
    if (int rc_e = eval_launch_pending(e)) return rc_e;
  if (n_rows < 0 || nnz < 0) return fail(FFM_E_INVALID, "negative n_rows / nnz");
  if (n_rows > e->max_rows || nnz > e->max_nnz)
    return fail(FFM_E_CAPACITY, "block exceeds max_batch_rows / max_batch_nnz");
  // (implicit_ones: rows in host memory, val == NULL -- every value is 1.0f, written on the device)
  if (!row_ptr || (nnz > 0 && (!feat || (!val && !implicit_ones)))) return fail(FFM_E_INVALID, "null CSR array");
  if (e->m.type == FFM_MODEL_FFM && nnz > 0 && !field && !implicit_fields)
    return fail(FFM_E_INVALID, "FFM requires the field array (libffm rows)");
  return FFM_OK;
}


// FFM evaluation rows one wave each (kernels_wave.h) where that kernel applies: a whole model on
// this device, a k with a lane shape (engine_select.h), the rows' entries within 64 KB of LDS per workgroup.
// A serving engine (engine_serve.h) has this kernel's twin and no other: create admitted only what it serves.
static bool launch_row_waves(ffm_engine *e, const Rows &rows, int row_cap, float *out, int output_prob) {
  const ModelDev &m = e->m;
  if (!serving(e) && (!e->predict_waves || m.type != FFM_MODEL_FFM || m.n_shards > 1 || m.field_start || m.own_n || m.lin_own)) return false;
  const RowWaveFn fn = row_wave_fn(m.lat_fmt, m.n_factors);
  if (!fn) return false;
  const int lds_cap = std::min(row_cap, kPredLdsCap);
  LAUNCH(e, serving(e) ? K_SERVE_ROW : K_PREDICT_ROW, fn, cdiv(rows.n_rows, kPredRows), 64 * kPredRows, pred_lds_bytes(lds_cap),
         m, rows, e->sc[e->cur], row_cap, lds_cap, out, output_prob);
  return true;
}

// An engine with a pair mask (engine_mask.h: set admitted only what this kernel serves) predicts every row through
// ffm_row_mask_kernel; a row beyond what a wave stages is flagged there, on a training engine too.
static void launch_row_mask(ffm_engine *e, const Rows &rows, int row_cap, float *out, int output_prob) {
  const ModelDev &m = e->m;
  const int lds_cap = std::min(row_cap, kPredLdsCap);
  LAUNCH(e, serving(e) ? K_SERVE_ROW : K_PREDICT_ROW, row_mask_fn(m.lat_fmt, m.n_factors), cdiv(rows.n_rows, kPredRows),
         64 * kPredRows, mask_lds_bytes(lds_cap), m, rows, e->sc[e->cur], row_cap, lds_cap, out, output_prob, e->d_pair_mask);
}

// row_cap: the longest row of the block where the caller knows it (rows that came in host memory), 0 = unknown
// (device callers: max_row_nnz).  The row kernels size their LDS by it, which decides how many rows a CU holds.
// weight: the block's sample weights (device) or null; only the launches that produce tmp_grad
// themselves (own_tg) take them -- otherwise tmp_grad_weighted_kernel does, after the logits are whole.
static void launch_row_kernel(ffm_engine *e, const Rows &rows, int row_cap, bool train, float *out, int output_prob, int own_tg = 0,
                              const float *weight = nullptr) {
  if (row_cap <= 0) row_cap = e->max_row_nnz;
  if (rows.n_rows == 0) return;
  if (!train && e->pair_mask_on) {  // (training is refused while a mask is set) -- the masked kernel and nothing else
    launch_row_mask(e, rows, row_cap, out, output_prob);
    return;
  }
  if (serving(e)) {  // (predict only: every training entry point is refused) -- its own kernel and nothing else
    launch_row_waves(e, rows, row_cap, out, output_prob);
    return;
  }
  // (the kernels recompute the same terms capacity from the same arguments)
  const int terms_cap = e->m.type == FFM_MODEL_FM ? row_terms_cap(2, 0, e->m.n_factors)
                        : row_terms_cap(row_cap, e->m.n_shards > 1 ? e->m.rec_slots : 0, 0);
  const size_t shmem = row_lds_bytes(row_cap, e->m.n_fields, terms_cap);
  const int kid = train ? K_ROW : K_PREDICT_ROW;
  if (e->m.type == FFM_MODEL_FM && e->m.n_factors <= 64) {
    // one wave per row, lane = factor (kernels_fm.h)
    if (train) e->singles_in_row = own_tg != 0;
    const int grid = cdiv(rows.n_rows, kFmRowsPerBlock);
    if (train && own_tg && weight) LAUNCH(e, kid, fm_row_wave_fn<const float *>(train), grid, 64 * kFmRowsPerBlock, 0, e->m, rows, e->sc[e->cur], row_cap, out, output_prob, own_tg, weight);
    else LAUNCH(e, kid, fm_row_wave_fn<>(train), grid, 64 * kFmRowsPerBlock, 0, e->m, rows, e->sc[e->cur], row_cap, out, output_prob, train ? own_tg : 0);
  } else if (e->m.type == FFM_MODEL_FM) {
    if (train) e->singles_in_row = false;
    LAUNCH(e, kid, fm_row_fn(train), rows.n_rows, kRowThreads, shmem, e->m, rows, e->sc[e->cur], row_cap, out, output_prob);
  } else {
    const bool vec4 = e->m.n_factors > 0 && e->m.n_factors % 4 == 0;
    const int mr = row_cap;
    int refreshed = train && e->pre_refresh ? e->refresh_mode : 0;
    if (refreshed == 3 && !(own_tg && vec4)) refreshed = 2;
    if (train) e->singles_in_row = refreshed == 3;
    if (refreshed && rows.nnz > 0) {
      const int per = vec4 ? e->m.row_len / 4 : e->m.row_len;
      const int64_t items = static_cast<int64_t>(std::min(rows.nnz, e->max_nnz)) * per;
      const int grid = static_cast<int>(std::min<int64_t>((items + 255) / 256, 8192));
      LAUNCH(e, K_REFRESH, ffm_refresh_fn(vec4), grid, 256, 0, e->m, e->sc[e->cur], refreshed >= 2);
    }
    // LDS parking (round 6: of w; round 4 parked (n, z)): the first vectors of w that a row's refresh
    // computes for its once-only features stay in LDS, where the row's pair phase and its in-row update
    // read them instead of fetching them back through an L2 they have left by then (128 rows in flight
    // per XCD x 31 KB of once-only w is the whole 4 MB L2).  As many as fit beside the staging arrays in
    // a 24 KB LDS budget (six rows per CU, which the kernel's 80 VGPRs allow: C5 row kernel 477 us with
    // nothing parked, 450 with 24 KB, 478 with 30 KB = five rows, 535 with 32 KB = four;
    // profiles/r06_experiments.md), at most what the longest row of the block can use.  FFM_ROW_PARK=bytes
    // overrides (0: off; a parked vector is 16 bytes) and FFM_ROW_PARK_BUDGET=bytes replaces the 24 KB,
    // both read when the engine is created: test_row_kernel_lds_parking_is_bit_identical pins 0 / 96 /
    // 1024 bytes / the default, test_gpu_launch_geometry.py also 16 bytes (one vector), 96 bytes at 64
    // threads and a 48 KB budget (above 32 KB).
    //
    // Held (n, z) (kernels_row.h, HOLD): the in-row update takes the first HOLD vectors each thread refreshed
    // from registers.  HOLD is the smallest of 2 / 4 / 6 / 8 that covers the longest row's once-only vectors per
    // thread, at most kRowHoldDefault (the measured best: profiles/row_hold.md), so that short records (k = 4,
    // few fields) hold what they need and no more; FFM_ROW_HOLD=n (read when the engine is created) replaces
    // that count, 0 = the kernel that holds nothing.  The parking budget does not follow the occupancy of the
    // instantiation: more LDS per row at fewer rows per CU measured slower at every count.
    int hold = 0;
    if (refreshed == 3 && train && vec4 && own_tg) {
      const long long vecs = static_cast<long long>(row_cap) * (e->m.rec_slots * (e->m.n_factors / 4));
      const long long need = (vecs + e->row_threads - 1) / e->row_threads;
      const long long want = e->row_hold >= 0 ? e->row_hold : std::min<long long>(need, kRowHoldDefault);
      hold = want <= 0 ? 0 : want <= 2 ? 2 : want <= 4 ? 4 : want <= 6 ? 6 : 8;
    }
    int park = 0;
    size_t shmem_park = shmem;
    if (refreshed == 3) {
      const int park_env = e->row_park, budget_env = e->row_park_budget;
      const size_t base = (shmem + 15) & ~static_cast<size_t>(15), budget = budget_env > 0 ? budget_env : 24 * 1024;
      long long bytes = park_env >= 0 ? park_env : (base < budget ? static_cast<long long>(budget - base) : 0);
      bytes = std::min<long long>(bytes, 16ll * row_cap * (e->m.row_len / 4));
      bytes = std::min<long long>(bytes, static_cast<long long>(budget) - static_cast<long long>(std::min(base, budget)));
      park = static_cast<int>(std::max<long long>(0, bytes) / 16);
      if (park > 0) shmem_park = base + 16 * static_cast<size_t>(park);
    }
    // the template's WHOLE (engine_select.h): the general-k training kernel is always the WHOLE one and learns
    // from own_tg whether the logit is (a shard's is whole only after the all-reduce: own_tg = 0)
    const bool whole = train && (own_tg || !vec4);
    int last = park;  // the kernels' last argument: vectors parked when training ...
    if (!train && launch_row_waves(e, rows, row_cap, out, output_prob)) {
      // rows that may be longer than a wave stages (kernels_wave.h): the workgroup-per-row kernel
      // for those alone (its last argument: rows of at most that many entries are not its)
      if (row_cap <= kPredLdsCap) return;
      last = kPredLdsCap;
    }
    // (shmem_park == shmem and park == 0 unless refreshed == 3, the in-row update's kernel)
    if (weight && own_tg)
      LAUNCH(e, kid, ffm_row_fn<const float *>(train, vec4, whole, hold), rows.n_rows, e->row_threads, shmem_park, e->m, rows, e->sc[e->cur], mr, out, output_prob, refreshed, own_tg, 0, last, weight);
    else
      LAUNCH(e, kid, ffm_row_fn<>(train, vec4, whole, hold), rows.n_rows, e->row_threads, shmem_park, e->m, rows, e->sc[e->cur], mr, out, output_prob, refreshed, own_tg, 0, last);
  }
}

static bool same_block(const Rows &a, const Rows &b) {
  return a.n_rows == b.n_rows && a.nnz == b.nnz && a.row_ptr == b.row_ptr && a.field == b.field &&
         a.feat == b.feat && a.val == b.val;
}

// Zeroes the grouping's counters and per-row field masks (a kernel: hipMemsetAsync costs the
// submitting thread ~100 us per call here, a launch ~5).
__global__ __launch_bounds__(256) void group_clear_kernel(int *counters, int n_counters,
                                                          unsigned long long *rowmask, int n_mask, int *n_super) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  if (tid == 0) __hip_atomic_store(n_super, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  for (int i = tid; i < n_counters; i += stride) counters[i] = 0;
  for (int i = tid; i < n_mask; i += stride) rowmask[i] = 0ull;
}

// Groups `rows` by feature into scratch set `set` on stream `st`.
// timed = false: from the staging thread (no HIP-event bookkeeping of the profiler there).
static int launch_grouping(ffm_engine *e, int set, const Rows &rows, hipStream_t st, bool timed = true) {
  Scratch &sc = e->sc[set];
  ScopedTimer tm_all("grouping:all");
  {
    ScopedTimer tm_clear("grouping:clear");
    const int n_mask = rows.nnz > 0 && sc.rowmask ? 2 * rows.n_rows : 0;
    hipLaunchKernelGGL(group_clear_kernel, dim3(std::max(1, std::min(64, cdiv(n_mask, 1024)))), dim3(256), 0, st,
                       sc.counters, kNumCounters, sc.rowmask, n_mask, sc.n_super);
  }
  if (rows.nnz > 0) {
    const int nnz = rows.nnz;
    if (timed) LAUNCH_ON(e, st, K_GROUP_KEYS, group_keys_kernel, cdiv(nnz, kGroupThreads), kGroupThreads, 0, e->m, rows, sc, e->max_row_nnz);
    else hipLaunchKernelGGL(group_keys_kernel, dim3(cdiv(nnz, kGroupThreads)), dim3(kGroupThreads), 0, st, e->m, rows, sc, e->max_row_nnz);
    if (timed) e->prof_begin(K_GROUP_SORT, st);
    {
      ScopedTimer tm_sort("grouping:sort");
      size_t bytes = e->sort_tmp_bytes;
      if (e->range_sort) {
        const size_t n_al = (static_cast<size_t>(nnz) + 63) & ~static_cast<size_t>(63);
        unsigned char *tmp = static_cast<unsigned char *>(e->d_sort_tmp[set]);
        RangeSortJob job{sc.key, sc.skey, sc.occ, reinterpret_cast<unsigned *>(tmp), reinterpret_cast<int *>(tmp + 4 * n_al),
                         e->d_sort_start, nnz, e->n_sort_ranges, static_cast<unsigned>(e->m.n_feats),
                         e->m.sort_start ? sc.counters + CNT_IRREGULAR : nullptr};
        hipLaunchKernelGGL(group_sort_ranges_kernel, dim3(e->n_sort_ranges), dim3(kSortThreads), 0, st, job);
      } else if (e->own_sort) {
        const size_t n_al = (static_cast<size_t>(nnz) + 63) & ~static_cast<size_t>(63);
        unsigned char *tmp = static_cast<unsigned char *>(e->d_sort_tmp[set]);
        SortJob job{sc.key, sc.skey, sc.occ, reinterpret_cast<unsigned *>(tmp), reinterpret_cast<int *>(tmp + 4 * n_al),
                    reinterpret_cast<unsigned *>(tmp + 8 * n_al), sc.counters + CNT_SORT_BAR,
                    sc.counters + CNT_ERROR, sc.err, nnz, static_cast<int>((e->sort_bits + 7) / 8)};
        hipLaunchKernelGGL(group_sort_kernel, dim3(sort_grid(nnz, e->sort_grid_cap)), dim3(kSortThreads), 0, st, job);
      } else
      HIP_TRY(rocprim::radix_sort_pairs<GroupSortConfig>(e->d_sort_tmp[set], bytes, sc.key, sc.skey,
                                        rocprim::counting_iterator<int>(0), sc.occ,
                                        static_cast<size_t>(nnz), 0u, e->sort_bits, st));
    }
    if (timed) e->prof_end(st);
    if (timed) LAUNCH_ON(e, st, K_GROUP_FINISH, group_finish_kernel, cdiv(nnz, kFinishThreads), kFinishThreads, 0, e->m, rows, sc);
    else hipLaunchKernelGGL(group_finish_kernel, dim3(cdiv(nnz, kFinishThreads)), dim3(kFinishThreads), 0, st, e->m, rows, sc);
  }
  HIP_TRY(hipGetLastError());
  return FFM_OK;
}

// A look-ahead grouping in two halves: the bookkeeping (caller's thread, in call order) and the
// stream operations (whoever submits: the caller's thread or the staging thread, in the same order).
struct PrepPlan {
  int set = 0;
  bool wait_free = false;  // the set carried an earlier block: wait for its ev_set_free
  int ws = -1;             // start when this set's block has trained (-1: at once); ffm_engine::trained_set
  Rows rows{};
};
static int prepare_plan(ffm_engine *e, const Rows &rows, PrepPlan *pl) {
  if (e->has_pending) return fail(FFM_E_INVALID, "prepare between train_forward and train_update");
  if (e->n_prepared >= ffm_engine::kSets - 1) return fail(FFM_E_CAPACITY, "three prepared blocks are already waiting");
  const int set = (e->last_set + 1) % ffm_engine::kSets;
  pl->set = set;
  pl->rows = rows;
  pl->wait_free = e->set_used[set];
  // n_prepared == 1: the predecessor is prepared but not enqueued yet -> wait for the block
  // enqueued last; n_prepared == 0: the predecessor IS the block enqueued last -> the one before
  const int ws = e->trained_set[e->n_prepared >= 1 ? 0 : 1];
  pl->ws = ws >= 0 && ws != set ? ws : -1;
  // the set is in use from now on, also when this look-ahead ends up discarded: whoever takes the
  // set next must wait for ev_set_free (recorded when the block trains or the look-ahead is dropped)
  e->set_used[set] = true;
  e->last_set = set;
  e->prepared_set[e->n_prepared] = set;
  e->prepared_rows[e->n_prepared] = rows;
  e->n_prepared++;
  return FFM_OK;
}
static int prepare_submit(ffm_engine *e, const PrepPlan &pl, bool timed) {
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  if (pl.wait_free) HIP_TRY(hipStreamWaitEvent(e->prep, e->ev_set_free[pl.set], 0));
  if (pl.ws >= 0) HIP_TRY(hipStreamWaitEvent(e->prep, e->prep_after_row ? e->ev_row_done[pl.ws] : e->ev_set_free[pl.ws], 0));
  int rc = launch_grouping(e, pl.set, pl.rows, e->prep, timed);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(e->ev_grouped[pl.set], e->prep));
  return FFM_OK;
}

int ffm_engine_prepare_device(ffm_engine *e, int32_t n_rows, int32_t nnz, const int32_t *row_ptr,
                              const int32_t *field, const int32_t *feat, const float *val) {
  SERVE_REFUSE(e, "ffm_engine_prepare_device");
  MASK_REFUSE(e, "training");
  int rc = check_block(e, n_rows, nnz, row_ptr, field, feat, val);
  if (rc) return rc;
  if ((rc = e->drain())) return rc;  // (staged blocks' submissions come first on the prep stream)
  PrepPlan pl;
  if ((rc = prepare_plan(e, Rows{n_rows, nnz, row_ptr, field, feat, val, nullptr}, &pl))) return rc;
  return prepare_submit(e, pl, true);
}

// What a forward call is told by its caller about this one block (nothing of it outlives the call).
struct ForwardOpts {
  int row_cap = 0;             // the block's longest row where the caller knows it (launch_row_kernel)
  bool whole_step = false;     // forward + update in one call (train_batch_device, train_staged) ...
  float *logit_out = nullptr;  // ... whose row kernel, where it has the whole logit, writes the logits here
};

// weight: the block's sample weights (device, [n_rows]) or null; remembered with the pending block
static int train_forward_core(ffm_engine *e, const Rows &rows, const float *weight, float *partial_logit,
                              const ForwardOpts &opts) {
  ScopedTimer tm_fwd("train:forward");
  SERVE_REFUSE(e, "training");
  MASK_REFUSE(e, "training");
  const int32_t n_rows = rows.n_rows;
  int rc = check_block(e, n_rows, rows.nnz, rows.row_ptr, rows.field, rows.feat, rows.val);
  if (rc) return rc;
  if (n_rows > 0 && !rows.label) return fail(FFM_E_INVALID, "training needs labels");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  e->pending = rows;
  e->pending_weight = n_rows > 0 ? weight : nullptr;
  e->has_pending = true;
  // only train_batch_device has the whole logit in its row kernel (one shard, FFM / LR)
  e->own_tg_cur = opts.whole_step && e->m.n_shards == 1 &&
                  (e->m.type != FFM_MODEL_FM || e->m.n_factors <= 64);  // (FM: fm_row_wave_kernel)
  const bool use_prepared = e->n_prepared > 0 && same_block(e->prepared_rows[0], rows);
  if (e->n_prepared > 0 && !use_prepared) {
    // groupings made ahead for some other block: forget them all
    if ((rc = e->drain())) return rc;
    for (int i = 0; i < e->n_prepared; i++) HIP_TRY(hipEventRecord(e->ev_set_free[e->prepared_set[i]], e->prep));
    e->n_prepared = 0;
  }
  e->cur_prepared = use_prepared;
  if (use_prepared) {
    e->cur = e->prepared_set[0];
    for (int i = 1; i < e->n_prepared; i++) {
      e->prepared_set[i - 1] = e->prepared_set[i];
      e->prepared_rows[i - 1] = e->prepared_rows[i];
    }
    e->n_prepared--;
    HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_grouped[e->cur], 0));
  } else {
    e->cur = (e->last_set + 1) % ffm_engine::kSets;
    e->last_set = e->cur;
    if (e->set_used[e->cur]) HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_set_free[e->cur], 0));
    rc = launch_grouping(e, e->cur, rows, e->stream);
    if (rc) return rc;
  }
  e->set_used[e->cur] = true;
  launch_row_kernel(e, rows, opts.row_cap, true, e->own_tg_cur ? opts.logit_out : nullptr, 0, e->own_tg_cur ? 1 : 0, e->pending_weight);
  if (e->prep_after_row) HIP_TRY(hipEventRecord(e->ev_row_done[e->cur], e->stream));
  if (partial_logit && n_rows > 0)
    HIP_TRY(hipMemcpyAsync(partial_logit, e->sc[e->cur].logit, sizeof(float) * n_rows, hipMemcpyDeviceToDevice, e->stream));
  HIP_TRY(hipGetLastError());
  return FFM_OK;
}

int ffm_engine_train_forward_device(ffm_engine *e, int32_t n_rows, int32_t nnz,
                                    const int32_t *row_ptr, const int32_t *field,
                                    const int32_t *feat, const float *val, const int32_t *label,
                                    float *partial_logit) {
  return train_forward_core(e, Rows{n_rows, nnz, row_ptr, field, feat, val, label}, nullptr, partial_logit, ForwardOpts{});
}
int ffm_engine_train_forward_device_weighted(ffm_engine *e, int32_t n_rows, int32_t nnz,
                                             const int32_t *row_ptr, const int32_t *field,
                                             const int32_t *feat, const float *val, const int32_t *label,
                                             const float *weight, float *partial_logit) {
  return train_forward_core(e, Rows{n_rows, nnz, row_ptr, field, feat, val, label}, weight, partial_logit, ForwardOpts{});
}

int ffm_engine_train_update_device(ffm_engine *e, const float *logit, float *logit_out,
                                   double *loss_sum_out) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  SERVE_REFUSE(e, "training");
  MASK_REFUSE(e, "training");
  if (!e->has_pending) return fail(FFM_E_INVALID, "train_update without a preceding train_forward");
  ScopedTimer tm_upd("train:update");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  const Rows rows = e->pending;
  e->has_pending = false;
  const float *lg = logit ? logit : e->sc[e->cur].logit;
  const bool own_tg = e->own_tg_cur && !logit;
  // progressive validation: the block's whole pre-update logits into the train channel (when it is on)
  launch_metric(e, FFM_METRIC_TRAIN, rows.n_rows, lg, 0, rows.label);
  launch_keyed(e, FFM_METRIC_TRAIN, rows, lg, 0);
  if (rows.n_rows > 0 && !own_tg) {
    if (e->pending_weight)
      LAUNCH(e, K_TMP_GRAD, tmp_grad_weighted_kernel, cdiv(rows.n_rows, 256), 256, 0, rows.n_rows, lg, rows.label, e->pending_weight, e->sc[e->cur].tg, e->sc[e->cur].loss, logit_out);
    else
      LAUNCH(e, K_TMP_GRAD, tmp_grad_kernel, cdiv(rows.n_rows, 256), 256, 0, rows.n_rows, lg, rows.label, e->sc[e->cur].tg, e->sc[e->cur].loss, logit_out);
  }
  e->pending_weight = nullptr;
  // Everything below runs on the main stream: the update has no long dependent chains (every
  // accumulator is folded by reductions, kernels_fold.h), so nothing needs a queue of its own.
  // FM, whole step: fm_row_wave_kernel has applied the touches of the once-only features itself
  const int fm_in_row = e->m.type == FFM_MODEL_FM && own_tg && e->singles_in_row ? 1 : 0;
  // this shard folds the bias / runs a linear update when it owns the bias / any field's linear terms
  const bool lin_owner = e->m.bias_own != 0 || e->lin_any;
  const bool ffm = e->m.type == FFM_MODEL_FFM && rows.nnz > 0;
  const bool vec4 = e->m.n_factors % 4 == 0;
  const bool masks = e->sc[e->cur].cmask != nullptr;  // (n_fields <= 64)
  const int lin_blocks = rows.nnz > 0 ? std::min(cdiv(rows.nnz, kUpdThreads), 1024) : 0;
  const int side_blocks = lin_owner && rows.n_rows > 0 ? 1 + lin_blocks : 0;
  bool loss_done = false;
  if (ffm && vec4 && masks) {
    const int span4 = e->m.rec_slots * (e->m.n_factors / 4);  // 16-byte vectors of a stored record
    const bool flat = flat_pays(e, span4);
    // A shard's once-only features (their logit was only whole after the all-reduce) and, on compact
    // storage, its few-occurrence features have launches of their own: on the side stream, beside the
    // update launch (disjoint features; a rank's step is long, the two queue hops are not)
    const bool side_launches = !e->singles_in_row || flat;
    hipStream_t sst = side_launches && !e->serial ? e->aux3 : e->stream;
    if (sst != e->stream) {
      HIP_TRY(hipEventRecord(e->ev_fork, e->stream));
      HIP_TRY(hipStreamWaitEvent(sst, e->ev_fork, 0));
    }
    if (!e->singles_in_row) {  // (else: already applied by the row kernel)
      if (flat) LAUNCH_ON(e, sst, K_LATENT_UPDATE_SINGLE, ffm_update_single_flat_kernel, e->grid_single, kUpdThreads, 0, e->m, rows, e->sc[e->cur]);
      else LAUNCH_ON(e, sst, K_LATENT_UPDATE_SINGLE, update_single_fn(span4), e->grid_single, kUpdThreads, 0, e->m, rows, e->sc[e->cur]);
    }
    // (the few-occurrence launch further down: beside the longest features' second pass and join,
    // which are chains of dependent loads on an otherwise idle chip)
    // (the grouping counted the block's longest features into page-locked host memory; it ran blocks
    // ahead, so its event has usually completed and the count can be read: none -> no launches)
    bool supers = rows.nnz >= e->m.super_min;
    if (supers && e->super_flag_ok && e->cur_prepared) {
      // The count is there once the block's grouping has run -- blocks ago in device time, so this wait
      // is over at once unless the caller is several steps ahead of the device, which it then stops
      // being (two steps stay queued).  Rounds 4-5 only QUERIED the event: a caller that ran ahead (a
      // zero-copy loop never blocks) found it pending in most steps and paid the two empty launches
      // and their gaps, ~30 us per C5 step (profiles/r06_experiments.md section 9).
      if (e->super_wait) HIP_TRY(hipEventSynchronize(e->ev_grouped[e->cur]));
      if (hipEventQuery(e->ev_grouped[e->cur]) == hipSuccess && e->h_super[e->cur] == 0) supers = false;
    }
    // (... and only then is the few-occurrence kernel worth deferring: a block without such features -- the
    // strong-scaling leg's 8192 rows -- has no second pass to run it beside: 0.349 -> 0.341 ms)
    const bool few_late = flat && sst != e->stream && supers;
    if (flat && !few_late) LAUNCH_ON(e, sst, K_LATENT_UPDATE_FEW, ffm_update_small_flat_kernel, e->grid_small, kUpdThreads, 0, e->m, rows, e->sc[e->cur], 1);
    if (sst != e->stream && !few_late) HIP_TRY(hipEventRecord(e->ev_join, sst));
    // (the ranges' sizes are kept in 256-thread units and scaled to the launch's workgroup size)
    // One launch, or three side by side: the one launch runs every range at the register / LDS footprint
    // of the hungriest (3 waves per SIMD at k = 16); side by side the few-occurrence range gets 4 and
    // the ranges overlap as the dispatcher finds room -- C5 resident step 1.005 -> 0.95-0.97 ms, but a
    // 4096 x 8 block 0.15 -> 0.21 ms (two more launches and a fork / join on a 100 us phase), and a
    // shard's rank (its once-only and few-occurrence launches already sit on the side queue) 1.71 ->
    // 1.77 ms.
    const int split = e->update_split >= 0 ? e->update_split
                      : (!side_launches && static_cast<int64_t>(rows.nnz) * e->m.n_factors >= (1ll << 20) ? 2 : 0);
    // (small blocks of a whole model, k >= 16: eight waves per workgroup -- kernels_tile.h kWideWaves)
    const int nf = tile_nf(e);
    const bool wide = nf == 1 && !side_launches && split == 0 && rows.nnz < e->wide_max_nnz;
    const int wpb = wide ? kWideWaves : tile_waves(nf), scale = wpb / kUpdWaves, threads = 64 * wpb;
    const size_t lds = tile_lds_bytes(nf, wpb);
    // (the few-occurrence launch of the three side by side has no tiles: only its staging of the touches' rows,
    // and that only where a block of this engine can be staged -- else it launches without dynamic LDS)
    const size_t few_lds = few_stage_possible(e->m) ? few_stage_bytes(wpb, e->m.n_fields) : 0;
    // (... and to the block: a workgroup that finds its range's lists empty still costs a dispatch and
    // a few dependent loads -- 4100 of them were a fifth of a 4096 x 8 block's update)
    auto sized = [&](int grid, int per_wg, int least) { return std::max(least, std::min(grid, cdiv(rows.nnz, per_wg))); };
    const int nt = cdiv(sized(e->grid_hot, 32, 64), scale), ns = flat ? 0 : cdiv(sized(e->grid_small, 128, 64), scale);
    const int nw = cdiv(sized(e->grid_walk, 1024, 16), scale);
    const int ng = rows.nnz >= kGiantMin ? sized(e->grid_giant, 256, 32) : 0;  // workgroups that fold giant features together
    const int order = e->update_order;  // (which of the three big ranges the dispatcher sees first)
    const int lb = loss_sum_out ? loss_grid(rows.n_rows) : 0;
    const int side = side_blocks > 0 ? 1 + cdiv(lin_blocks, scale) : 0;
    // One launch of the ranges `kinds` (the arguments of every other range are 0), from the instantiation
    // that carries those ranges alone: nf = 1 for k >= 16, 2 for k = 8 / 12, 4 for k = 4 (engine_select.h).
    // few_only is 1: a once-only feature is its row's or the once-only kernel's, never the few-occurrence range's.
    auto launch_ranges = [&](hipStream_t st, int kid, int kinds, size_t shm, int ord) {
      const int a_side = kinds & UPD_SIDE ? side : 0, a_ng = kinds & UPD_GIANT ? ng : 0, a_nt = kinds & UPD_HOT ? nt : 0;
      const int a_ns = kinds & UPD_FEW ? ns : 0, a_nw = kinds & UPD_REST ? nw : 0, a_lb = kinds & UPD_REST ? lb : 0;
      LAUNCH_ON(e, st, kid, update_all_fn(nf, kinds, wpb), a_side + a_ng + a_nt + a_ns + a_nw + a_lb, threads, shm, e->m, rows,
                e->sc[e->cur], a_side, a_ng, a_nt, a_ns, 1, a_nw, a_lb, loss_sum_out, e->d_loss_part, ord);
    };
    if (split == 2 && !e->serial) {  // side by side: few on aux3, giant on aux4
      HIP_TRY(hipEventRecord(e->ev_fork2, e->stream));
      if (ns + nw + lb > 0) {
        HIP_TRY(hipStreamWaitEvent(e->aux3, e->ev_fork2, 0));
        launch_ranges(e->aux3, K_LATENT_UPDATE_FEW, UPD_FEW | UPD_REST, few_lds, order);
        HIP_TRY(hipEventRecord(e->ev_join, e->aux3));
      }
      if (ng > 0) {
        HIP_TRY(hipStreamWaitEvent(e->aux4, e->ev_fork2, 0));
        launch_ranges(e->aux4, K_LATENT_UPDATE_GIANT, UPD_GIANT, lds, order);
        HIP_TRY(hipEventRecord(e->ev_join2, e->aux4));
      }
      launch_ranges(e->stream, K_LATENT_UPDATE, UPD_HOT | UPD_SIDE, lds, 1);
      if (ns + nw + lb > 0) HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_join, 0));
      if (ng > 0) HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_join2, 0));
    } else if (split) {  // (timing aid: one launch per range, each under a name of its own)
      if (ng > 0) launch_ranges(e->stream, K_LATENT_UPDATE_GIANT, UPD_GIANT, lds, order);
      launch_ranges(e->stream, K_LATENT_UPDATE, UPD_HOT | UPD_SIDE, lds, order);
      if (ns > 0) launch_ranges(e->stream, K_LATENT_UPDATE_FEW, UPD_FEW, lds, order);
      launch_ranges(e->stream, K_LATENT_UPDATE_WALK, UPD_REST, lds, order);
    } else if (ns == 0) {
      // a shard: its few-occurrence features have a kernel of their own, and without that range's registers
      // the launch holds four waves per SIMD (128 VGPRs, 11 spilled) instead of three at 143: an emulated
      // 8-GPU rank's step 1.658 -> 1.619 ms
      launch_ranges(e->stream, K_LATENT_UPDATE, UPD_ALL & ~UPD_FEW, lds, order);
    } else {  // (wide: the eight-wave instantiation, by wpb)
      launch_ranges(e->stream, K_LATENT_UPDATE, UPD_ALL, lds, order);
    }
    if (few_late) {
      HIP_TRY(hipEventRecord(e->ev_fork2, e->stream));
      HIP_TRY(hipStreamWaitEvent(sst, e->ev_fork2, 0));
      LAUNCH_ON(e, sst, K_LATENT_UPDATE_FEW, ffm_update_small_flat_kernel, e->grid_small, kUpdThreads, 0, e->m, rows, e->sc[e->cur], 1);
      HIP_TRY(hipEventRecord(e->ev_join, sst));
    }
    if (supers) {
      // the longest features' ranges: second pass (root differences) and the join of their tiles
      const int gg = e->grid_giant;
      e->prof_begin(K_LATENT_UPDATE_GIANT, e->stream);
      hipLaunchKernelGGL(update_super_b_fn(nf), dim3(gg), dim3(kUpdThreads), 0, e->stream, e->m, rows, e->sc[e->cur]);
      hipLaunchKernelGGL(ffm_update_super_join_kernel, dim3(gg), dim3(kUpdThreads), 0, e->stream, e->m, e->sc[e->cur]);
      e->prof_end(e->stream);
    }
    if (sst != e->stream) HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_join, 0));
    loss_done = loss_sum_out != nullptr;
  } else {
    if (side_blocks > 0 && e->m.type != FFM_MODEL_FM) {
      LAUNCH(e, K_BIAS_UPDATE, bias_update_kernel, 1, kUpdThreads, 0, e->m, rows.n_rows, e->sc[e->cur]);
      if (rows.nnz > 0)
        LAUNCH(e, K_LINEAR_UPDATE, linear_update_kernel, lin_blocks, kUpdThreads, 0, e->m, rows, e->sc[e->cur], 0);
    }
    if (ffm) {
      // n_factors % 4 != 0, or more than 64 fields (no field masks: every slot keeps the row-order
      // walk): the general owner for every feature, the once-only ones included
      LAUNCH(e, K_LATENT_UPDATE, ffm_update_generic_kernel, 2048, kUpdThreads, 0, e->m, rows, e->sc[e->cur], 0);
    } else if (e->m.type == FFM_MODEL_FM) {
      if (rows.nnz > 0) {
        LAUNCH(e, K_LATENT_UPDATE, fm_update_kernel, side_blocks + 2048, kUpdThreads, 0, e->m, rows, e->sc[e->cur], fm_in_row, side_blocks);
        if (rows.nnz >= e->m.giant_min)  // the giant features' segments joined
          LAUNCH(e, K_LATENT_UPDATE_GIANT, fm_update_join_kernel, 256, kUpdThreads, 0, e->m, e->sc[e->cur]);
      }
      else if (side_blocks > 0)
        LAUNCH(e, K_BIAS_UPDATE, bias_update_kernel, 1, kUpdThreads, 0, e->m, rows.n_rows, e->sc[e->cur]);
    }
  }
  if (loss_sum_out && !loss_done)
    LAUNCH(e, K_LOSS_SUM, loss_sum_kernel, loss_grid(rows.n_rows), 256, 0, rows.n_rows, e->sc[e->cur].loss, loss_sum_out, e->d_loss_part);
  HIP_TRY(hipEventRecord(e->ev_set_free[e->cur], e->stream));
  e->trained_set[1] = e->trained_set[0];
  e->trained_set[0] = e->cur;
  if (e->cur_slot >= 0) {  // a staged block: its staging slot may be refilled from here on
    e->slots[e->cur_slot].free_ev = e->ev_set_free[e->cur];  // (not recorded again before the slot's next turn: kSets blocks later)
    e->cur_slot = -1;
  }
  HIP_TRY(hipGetLastError());
  return FFM_OK;
}

// The whole step on a block in HBM; row_cap as launch_row_kernel takes it.
static int train_batch_core(ffm_engine *e, const Rows &rows, const float *weight, float *logit_out, double *loss_sum_out,
                            int row_cap) {
  if (e && e->m.n_shards > 1)
    return fail(FFM_E_INVALID, "sharded engines train with train_forward + all-reduce + train_update");
  int rc = train_forward_core(e, rows, weight, nullptr, ForwardOpts{row_cap, true, logit_out});
  if (rc) return rc;
  return ffm_engine_train_update_device(e, nullptr, logit_out, loss_sum_out);
}
int ffm_engine_train_batch_device_weighted(ffm_engine *e, int32_t n_rows, int32_t nnz,
                                           const int32_t *row_ptr, const int32_t *field,
                                           const int32_t *feat, const float *val, const int32_t *label,
                                           const float *weight, float *logit_out, double *loss_sum_out) {
  return train_batch_core(e, Rows{n_rows, nnz, row_ptr, field, feat, val, label}, weight, logit_out, loss_sum_out, 0);
}
int ffm_engine_train_batch_device(ffm_engine *e, int32_t n_rows, int32_t nnz,
                                  const int32_t *row_ptr, const int32_t *field,
                                  const int32_t *feat, const float *val, const int32_t *label,
                                  float *logit_out, double *loss_sum_out) {
  return ffm_engine_train_batch_device_weighted(e, n_rows, nnz, row_ptr, field, feat, val, label, nullptr, logit_out,
                                                loss_sum_out);
}

// Prediction of a block in HBM; row_cap as launch_row_kernel takes it.
static int predict_core(ffm_engine *e, const Rows &rows, int32_t output_prob, float *out, double *loss_sum_out, int row_cap) {
  const int32_t n_rows = rows.n_rows;
  const int32_t *const label = rows.label;
  int rc = check_block(e, n_rows, rows.nnz, rows.row_ptr, rows.field, rows.feat, rows.val);
  if (rc) return rc;
  if (e->m.n_shards > 1 && (label || output_prob || loss_sum_out))
    return fail(FFM_E_INVALID, "a sharded engine predicts partial logits only (label = NULL, output_prob = 0, "
                               "no loss): sum them across shards, then ffm_engine_predict_finish_device");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  launch_row_kernel(e, rows, row_cap, false, out ? out : e->d_out, output_prob);
  if (label) launch_metric(e, FFM_METRIC_EVAL, n_rows, out ? out : e->d_out, output_prob, label);
  if (label) launch_keyed(e, FFM_METRIC_EVAL, rows, out ? out : e->d_out, output_prob);
  if (loss_sum_out && label)
    LAUNCH(e, K_LOSS_SUM, loss_sum_kernel, loss_grid(n_rows), 256, 0, n_rows, e->sc[e->cur].loss, loss_sum_out, e->d_loss_part);
  HIP_TRY(hipGetLastError());
  return FFM_OK;
}
int ffm_engine_predict_batch_device(ffm_engine *e, int32_t n_rows, int32_t nnz,
                                    const int32_t *row_ptr, const int32_t *field,
                                    const int32_t *feat, const float *val, const int32_t *label,
                                    int32_t output_prob, float *out, double *loss_sum_out) {
  return predict_core(e, Rows{n_rows, nnz, row_ptr, field, feat, val, label}, output_prob, out, loss_sum_out, 0);
}

int ffm_engine_predict_finish_device(ffm_engine *e, int32_t n_rows, const float *logit,
                                     const int32_t *label, int32_t output_prob, float *out,
                                     double *loss_sum_out) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  if (n_rows < 0 || n_rows > e->max_rows) return fail(FFM_E_CAPACITY, "n_rows out of range");
  if (n_rows > 0 && !logit) return fail(FFM_E_INVALID, "null logit array");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  // (from the logits, ahead of the kernel that may overwrite them: `out` may alias `logit` or be NULL)
  if (label) launch_metric(e, FFM_METRIC_EVAL, n_rows, logit, 0, label);
  if (n_rows > 0)
    LAUNCH(e, K_TMP_GRAD, predict_finish_kernel, cdiv(n_rows, 256), 256, 0, n_rows, logit, label, output_prob, out, e->sc[e->cur].loss);
  if (loss_sum_out) {
    if (label) LAUNCH(e, K_LOSS_SUM, loss_sum_kernel, loss_grid(n_rows), 256, 0, n_rows, e->sc[e->cur].loss, loss_sum_out, e->d_loss_part);
    else HIP_TRY(hipMemsetAsync(loss_sum_out, 0, sizeof(double), e->stream));
  }
  HIP_TRY(hipGetLastError());
  return FFM_OK;
}

// Checks one block of host arrays; returns its nnz and its longest row.
// *field: null afterwards on LR / FM, whose rows have no fields (libsvm: src/data/parser.cpp:20 gives every
// entry field 0) -- a field array the caller passes along is not uploaded: a third of the block's bytes over PCIe.
// hold_eval: as check_block takes it.
// implicit_fields (the staged entry points, FFM, field == NULL): every row must then hold exactly one
// entry per field, entry j of a row being field j's -- the upload kernel writes the field array itself.
// Rows in host memory may always come without values (val == NULL: every value is 1.0f): the array is written
// on the device, by the upload kernel (engine_stage.h) or, on the synchronous calls, by stage_block's fill.
static int validate_host_block(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr,
                               const int32_t **field_io, const int32_t *feat, const float *val,
                               int32_t *nnz_out, int *longest_out, bool implicit_fields = false, bool hold_eval = false) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  if (e->m.type != FFM_MODEL_FFM) *field_io = nullptr;
  const int32_t *const field = *field_io;
  if (n_rows < 0) return fail(FFM_E_INVALID, "negative n_rows");
  if (!row_ptr) return fail(FFM_E_INVALID, "null row_ptr");
  if (n_rows > e->max_rows) return fail(FFM_E_CAPACITY, "block exceeds max_batch_rows");
  if (row_ptr[0] != 0) return fail(FFM_E_INVALID, "row_ptr[0] must be 0");
  for (int r = 0; r < n_rows; r++)
    if (row_ptr[r + 1] < row_ptr[r]) return fail(FFM_E_INVALID, "row_ptr must be non-decreasing");
  const int32_t nnz = row_ptr[n_rows];
  int rc = check_block(e, n_rows, nnz, row_ptr, field, feat, val, implicit_fields, true, hold_eval);
  if (rc) return rc;
  if (implicit_fields && !field && e->m.type == FFM_MODEL_FFM)
    for (int r = 0; r < n_rows; r++)
      if (row_ptr[r + 1] - row_ptr[r] != e->m.n_fields)
        return fail(FFM_E_INVALID, "rows without a field array need exactly one entry per field");
  int longest = 1;
  for (int r = 0; r < n_rows; r++) {
    if (row_ptr[r + 1] - row_ptr[r] > e->max_row_nnz)
      return fail(FFM_E_CAPACITY, "a row has more entries than max_row_nnz");
    longest = std::max(longest, row_ptr[r + 1] - row_ptr[r]);
  }
  *nnz_out = nnz;
  *longest_out = longest;
  return FFM_OK;
}

// Sample weights handed over in host memory: finite and >= 0, checked on the caller's thread before
// anything of the block is queued (the device entry points look at weights no more than at val).
static int validate_host_weights(int32_t n_rows, const float *weight) {
  for (int r = 0; r < n_rows; r++)
    if (!(weight[r] >= 0.0f) || std::isinf(weight[r]))
      return fail(FFM_E_INVALID, "sample weight of row " + std::to_string(r) + " is " +
                                     (std::isnan(weight[r]) ? "NaN" : std::isinf(weight[r]) ? "infinite" : "negative") +
                                     ": weights must be finite and >= 0");
  return FFM_OK;
}

// The synchronous calls' share of val == NULL (the staged calls': the upload kernel, engine_stage.h): n values
// of 1.0f written in place of the array's copy, four per lane as one 16-byte vector, the last n % 4 singly.
__global__ __launch_bounds__(256) void fill_ones_kernel(float *val, unsigned n) {
  const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  const unsigned n4 = n >> 2;
  const float4 ones4 = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
  for (unsigned i = tid; i < n4; i += stride) reinterpret_cast<float4 *>(val)[i] = ones4;
  if (tid < (n & 3u)) val[(n4 << 2) + tid] = 1.0f;
}

// The synchronous calls' copy of a host block into the engine's own device arrays, on the main stream.
// Returns the block as the _device cores take it (*dev) and its longest row (*row_cap_out).
static int stage_block(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr, const int32_t *field,
                       const int32_t *feat, const float *val, const int32_t *label, Rows *dev, int *row_cap_out,
                       const float *weight = nullptr) {
  int32_t nnz = 0;
  int longest = 1;
  int rc = validate_host_block(e, n_rows, row_ptr, &field, feat, val, &nnz, &longest);
  if (rc) return rc;
  if (weight) {
    if ((rc = validate_host_weights(n_rows, weight))) return rc;
    // (allocated by the first weighted block: an engine that never sees weights holds nothing for them)
    if (!e->d_weight && (rc = e->alloc(&e->d_weight, static_cast<size_t>(e->max_rows)))) return rc;
  }
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  HIP_TRY(hipMemcpyAsync(e->d_row_ptr, row_ptr, sizeof(int32_t) * (n_rows + 1), hipMemcpyHostToDevice, e->stream));
  if (nnz > 0) {
    if (field) HIP_TRY(hipMemcpyAsync(e->d_field, field, sizeof(int32_t) * nnz, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->d_feat, feat, sizeof(int32_t) * nnz, hipMemcpyHostToDevice, e->stream));
    if (val) HIP_TRY(hipMemcpyAsync(e->d_val, val, sizeof(float) * nnz, hipMemcpyHostToDevice, e->stream));
    else  // (no values came: a kernel writes them in place of the copy)
      hipLaunchKernelGGL(fill_ones_kernel, dim3(std::max(1, std::min(256, cdiv(cdiv(nnz, 4), 256)))), dim3(256), 0, e->stream,
                         e->d_val, static_cast<unsigned>(nnz));
  }
  if (label && n_rows > 0)
    HIP_TRY(hipMemcpyAsync(e->d_label, label, sizeof(int32_t) * n_rows, hipMemcpyHostToDevice, e->stream));
  if (weight && n_rows > 0)
    HIP_TRY(hipMemcpyAsync(e->d_weight, weight, sizeof(float) * n_rows, hipMemcpyHostToDevice, e->stream));
  // FFM_FLAG_HASH_IDS: the ids in place, behind their copy and ahead of every kernel that reads them
  if (e->hash_ids) launch_hash_ids(e, e->stream, nnz, field ? e->d_field : nullptr, e->d_feat, e->d_feat, e->d_val);
  *dev = Rows{n_rows, nnz, e->d_row_ptr, field ? e->d_field : nullptr, e->d_feat, e->d_val, label ? e->d_label : nullptr};
  // FFM_FLAG_NORM_ROWS: the values in place, behind the ids they are kept by and ahead of every kernel that reads them
  if (e->norm_rows_on) launch_normalize_rows(e, e->stream, norm_job(e, *dev, e->d_val));
  *row_cap_out = longest;
  return FFM_OK;
}

int ffm_engine_train_batch_weighted(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr,
                                    const int32_t *field, const int32_t *feat, const float *val,
                                    const int32_t *label, const float *weight, float *logit_out,
                                    double *loss_sum_out) {
  SERVE_REFUSE(e, "training");  // (before anything of the block is copied)
  MASK_REFUSE(e, "training");
  Rows dev{};
  int row_cap = 0;
  int rc = stage_block(e, n_rows, row_ptr, field, feat, val, label, &dev, &row_cap, weight);
  if (rc) return rc;
  if (n_rows > 0 && !label) return fail(FFM_E_INVALID, "training needs labels");
  dev.label = e->d_label;  // (also for a block of no rows that came without labels)
  if ((rc = train_batch_core(e, dev, weight ? e->d_weight : nullptr, e->d_out, e->d_loss_sum, row_cap))) return rc;
  if (logit_out && n_rows > 0)
    HIP_TRY(hipMemcpyAsync(logit_out, e->d_out, sizeof(float) * n_rows, hipMemcpyDeviceToHost, e->stream));
  if (loss_sum_out)
    HIP_TRY(hipMemcpyAsync(loss_sum_out, e->d_loss_sum, sizeof(double), hipMemcpyDeviceToHost, e->stream));
  return check_device_errors(e);
}
int ffm_engine_train_batch(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr,
                           const int32_t *field, const int32_t *feat, const float *val,
                           const int32_t *label, float *logit_out, double *loss_sum_out) {
  return ffm_engine_train_batch_weighted(e, n_rows, row_ptr, field, feat, val, label, nullptr, logit_out, loss_sum_out);
}

int ffm_engine_predict_batch(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr,
                             const int32_t *field, const int32_t *feat, const float *val,
                             const int32_t *label, int32_t output_prob, float *out,
                             double *loss_sum_out) {
  Rows dev{};
  int row_cap = 0;
  int rc = stage_block(e, n_rows, row_ptr, field, feat, val, label, &dev, &row_cap);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(e->sc[e->cur].counters, 0, kNumCounters * sizeof(int), e->stream));
  if ((rc = predict_core(e, dev, output_prob, e->d_out, e->d_loss_sum, row_cap))) return rc;
  if (out && n_rows > 0)
    HIP_TRY(hipMemcpyAsync(out, e->d_out, sizeof(float) * n_rows, hipMemcpyDeviceToHost, e->stream));
  if (loss_sum_out) {
    if (label) HIP_TRY(hipMemcpyAsync(loss_sum_out, e->d_loss_sum, sizeof(double), hipMemcpyDeviceToHost, e->stream));
    else *loss_sum_out = 0.0;
  }
  return check_device_errors(e);
}
