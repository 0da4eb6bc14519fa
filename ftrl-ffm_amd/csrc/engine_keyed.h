// engine_keyed.h -- keyed capture behind ffm_engine_metrics_*keyed* (include/ffm_engine.h "Metrics", keyed
// capture): one word per labelled row in HBM (keyed_capture_kernel), and at a read the words sorted, ranked
// per key and reduced to the per-key table on the engine's stream (kernels_keyed.h), averaged on the host
// (metrics_host.h).  Part of engine.hip's translation unit (included inside its extern "C" block).

// ---- keyed capture -------------------------------------------------------------------------

static constexpr int64_t kKeyedMaxRows = 1ll << 30;
static constexpr unsigned kKeyedSortMaxWg = 2048;  // workgroups of a sort pass at the most: [256][2048] counters

// One launch per labelled block and channel, only when the channel's capture is on.
static void launch_keyed(ffm_engine *e, int channel, const Rows &rows, const float *score, int is_prob) {
  const ffm_engine::KeyedChannel &ch = e->keyed[channel];
  if (!ch.on || rows.n_rows <= 0 || !rows.label) return;
  LAUNCH(e, K_KEYED_CAPTURE, keyed_capture_kernel, cdiv(rows.n_rows, kKeyedRowsPerWg), kKeyedThreads, 0, rows, e->m.n_feats,
         e->keyed_field, score, is_prob, ch.words, static_cast<unsigned long long>(e->keyed_capacity), ch.counters);
}

static int keyed_refuse(const ffm_engine *e) {
  if (ffm_metrics_host::keyed_shape_check(e->cfg.model_type, e->cfg.n_shards, e->in_group) == FFM_OK) return FFM_OK;
  return fail(FFM_E_UNSUPPORTED, "keyed capture: FFM engines of one shard outside a group only (LR and FM have no fields)");
}

int ffm_engine_metrics_key_field(ffm_engine *e, int32_t channel_mask, int32_t key_field, int64_t capacity_rows) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  if (int rc_r = keyed_refuse(e)) return rc_r;
  if (channel_mask < 0 || channel_mask > 3) return fail(FFM_E_INVALID, "channel_mask: bit 0 = eval, bit 1 = train");
  if (channel_mask != 0) {
    if (ffm_metrics_host::keyed_args_check(e->cfg.n_fields, key_field, capacity_rows) != FFM_OK)
      return fail(FFM_E_INVALID, "key_field must name a field and capacity_rows be positive");
    if (capacity_rows > kKeyedMaxRows) return fail(FFM_E_UNSUPPORTED, "capacity_rows above 2^30");
  }
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  // a deferred evaluation block belongs to the setting it was handed over under
  if (int rc_e = eval_launch_pending(e)) return rc_e;
  if (channel_mask == 0) {
    e->keyed[0].on = e->keyed[1].on = false;
    return FFM_OK;
  }
  const bool changed = key_field != e->keyed_field || capacity_rows != e->keyed_capacity;
  const size_t cap = static_cast<size_t>(capacity_rows);
  const size_t n_tab = static_cast<size_t>(std::min<int64_t>(capacity_rows, e->m.n_feats));
  if (int rc = e->grow(&e->keyed_scratch, &e->keyed_scratch_cap, cap)) return rc;
  if (int rc = e->grow(&e->keyed_tab, &e->keyed_tab_cap, 3 * n_tab)) return rc;
  if (int rc = e->grow(&e->keyed_tab_key, &e->keyed_tab_key_cap, n_tab)) return rc;
  if (int rc = e->grow(&e->keyed_rank_sums, &e->keyed_rank_sums_cap, (cap + kKeyedTile - 1) / kKeyedTile)) return rc;
  if (!e->keyed_hist) {
    if (int rc = e->alloc(&e->keyed_hist, 256 * static_cast<size_t>(kKeyedSortMaxWg))) return rc;
    if (int rc = e->alloc(&e->keyed_hist_sums, (256 * static_cast<size_t>(kKeyedSortMaxWg) + kKeyedScanTile - 1) / kKeyedScanTile)) return rc;
    if (int rc = e->alloc(&e->keyed_n_keys, 1)) return rc;
  }
  for (int c = 0; c < 2; c++) {
    ffm_engine::KeyedChannel &ch = e->keyed[c];
    const bool want = (channel_mask >> c) & 1;
    if (want) {
      // (a read may have swapped this buffer with a larger scratch buffer: never shrinks)
      if (int rc = e->grow(&ch.words, &ch.words_cap, cap)) return rc;
      if (!ch.counters)
        if (int rc = e->alloc(&ch.counters, KEYED_COUNTERS)) return rc;
      if (!ch.on || changed) HIP_TRY(hipMemsetAsync(ch.counters, 0, KEYED_COUNTERS * sizeof(unsigned long long), e->stream));
    }
    ch.on = want;
  }
  e->keyed_field = key_field;
  e->keyed_capacity = capacity_rows;
  return FFM_OK;
}

// The exclusive scan of a[0 .. n) in place: tile sums, one workgroup over the sums, apply.
static void keyed_scan_u32(ffm_engine *e, unsigned *a, unsigned n, unsigned *sums) {
  const unsigned tiles = (n + kKeyedScanTile - 1) / kKeyedScanTile;
  LAUNCH(e, K_KEYED_SORT_SCAN, keyed_scan_sums_kernel, tiles, kKeyedThreads, 0, a, n, sums);
  LAUNCH(e, K_KEYED_SORT_SCAN, keyed_scan_top_kernel<SumU32>, 1, kKeyedThreads, 0, sums, tiles);
  LAUNCH(e, K_KEYED_SORT_SCAN, keyed_scan_apply_kernel, tiles, kKeyedThreads, 0, a, n, sums);
}

// Sorts the channel's first n words ascending (afterwards ch.words holds them: the buffers swap roles after an
// odd number of passes).  The digits that cannot differ are skipped: bit 31, and the bits above the key's width.
static void keyed_sort(ffm_engine *e, ffm_engine::KeyedChannel &ch, unsigned n) {
  int key_bits = 0;
  while (key_bits < 31 && (1ll << key_bits) < static_cast<int64_t>(e->m.n_feats)) key_bits++;
  // workgroup w sorts words [w * chunk, (w + 1) * chunk): whole sub-tiles of 256, at most kKeyedSortMaxWg workgroups
  unsigned chunk = (n + kKeyedSortMaxWg - 1) / kKeyedSortMaxWg;
  chunk = std::max(1u, (chunk + kKeyedThreads - 1) / kKeyedThreads) * kKeyedThreads;
  const unsigned n_wg = (n + chunk - 1) / chunk;
  auto pass = [&](int shift, int bits) {
    const unsigned dmask = (1u << bits) - 1u;
    LAUNCH(e, K_KEYED_SORT_HIST, keyed_sort_hist_kernel, n_wg, kKeyedThreads, 0, ch.words, n, chunk, shift, dmask, e->keyed_hist);
    keyed_scan_u32(e, e->keyed_hist, 256u * n_wg, e->keyed_hist_sums);
    LAUNCH(e, K_KEYED_SORT_SCATTER, keyed_sort_scatter_kernel, n_wg, kKeyedThreads, 0, ch.words, e->keyed_scratch, n, chunk, shift,
           dmask, e->keyed_hist);
    std::swap(ch.words, e->keyed_scratch);
    std::swap(ch.words_cap, e->keyed_scratch_cap);
  };
  for (int shift = 0; shift < 31; shift += 8) pass(shift, std::min(8, 31 - shift));
  for (int s = 0; s < key_bits; s += 8) pass(32 + s, std::min(8, key_bits - s));
}

// What a read leaves on the host: the channel's counters, and the per-key table of its stored rows.
struct KeyedSnapshot {
  int64_t n_rows = 0, n_nan = 0, n_unkeyed = 0, n_overflow = 0;
  std::vector<int32_t> key;
  std::vector<unsigned long long> tab;  // [n_keys][3]: P, N, U2
};

static int keyed_snapshot(ffm_engine *e, int32_t channel, bool reset, KeyedSnapshot *snap) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  if (channel < 0 || channel > 1) return fail(FFM_E_INVALID, "channel: 0 = eval, 1 = train");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  if (int rc_e = eval_launch_pending(e)) return rc_e;
  ffm_engine::KeyedChannel &ch = e->keyed[channel];
  if (!ch.on) return fail(FFM_E_INVALID, "keyed capture is off on this channel (ffm_engine_metrics_key_field)");
  unsigned long long cnt[KEYED_COUNTERS] = {};
  HIP_TRY(hipMemcpyAsync(cnt, ch.counters, sizeof cnt, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const unsigned n = static_cast<unsigned>(std::min<unsigned long long>(cnt[KEYED_N_ASKED], static_cast<unsigned long long>(e->keyed_capacity)));
  snap->n_rows = n;
  snap->n_nan = static_cast<int64_t>(cnt[KEYED_N_NAN]);
  snap->n_unkeyed = static_cast<int64_t>(cnt[KEYED_N_UNKEYED]);
  snap->n_overflow = static_cast<int64_t>(cnt[KEYED_N_OVERFLOW]);
  unsigned n_keys = 0;
  if (n > 0) {
    keyed_sort(e, ch, n);
    const unsigned n_tab = static_cast<unsigned>(std::min<int64_t>(e->keyed_capacity, e->m.n_feats));
    const unsigned tiles = (n + kKeyedTile - 1) / kKeyedTile;
    HIP_TRY(hipMemsetAsync(e->keyed_tab, 0, 3 * sizeof(unsigned long long) * std::min(n, n_tab), e->stream));
    LAUNCH(e, K_KEYED_RANK, keyed_rank_sums_kernel, tiles, kKeyedThreads, 0, ch.words, n, e->keyed_rank_sums);
    LAUNCH(e, K_KEYED_RANK, keyed_scan_top_kernel<RankOp>, 1, kKeyedThreads, 0, e->keyed_rank_sums, tiles);
    LAUNCH(e, K_KEYED_RANK, keyed_rank_apply_kernel, tiles, kKeyedThreads, 0, ch.words, n, e->keyed_rank_sums, e->keyed_tab_key,
           e->keyed_tab, n_tab, e->keyed_n_keys);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&n_keys, e->keyed_n_keys, sizeof n_keys, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (n_keys > std::min(n, n_tab)) return fail(FFM_E_DEVICE, "keyed capture: more keys than the table holds");
  }
  try {
    snap->key.assign(n_keys, 0);
    snap->tab.assign(3 * static_cast<size_t>(n_keys), 0ull);
  } catch (const std::bad_alloc &) { return fail(FFM_E_NOMEM, "host allocation failed"); }
  if (n_keys > 0) {
    HIP_TRY(hipMemcpyAsync(snap->key.data(), e->keyed_tab_key, sizeof(int32_t) * n_keys, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(snap->tab.data(), e->keyed_tab, 3 * sizeof(unsigned long long) * n_keys, hipMemcpyDeviceToHost, e->stream));
  }
  if (reset) HIP_TRY(hipMemsetAsync(ch.counters, 0, sizeof cnt, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return FFM_OK;
}

int ffm_engine_metrics_from_keyed(const int64_t *pos, const int64_t *neg, const uint64_t *u2, int64_t n_keys,
                                  ffm_keyed_metrics *out) {
  const int rc = ffm_metrics_host::from_keyed(pos, neg, u2, n_keys, out);
  return rc ? fail(rc, "null array, null output or negative count") : FFM_OK;
}

// The snapshot's table as the three arrays the reduction takes.
static int keyed_columns(const KeyedSnapshot &s, std::vector<int64_t> *pos, std::vector<int64_t> *neg, std::vector<uint64_t> *u2) {
  const size_t nk = s.key.size();
  try {
    pos->resize(nk); neg->resize(nk); u2->resize(nk);
  } catch (const std::bad_alloc &) { return fail(FFM_E_NOMEM, "host allocation failed"); }
  for (size_t g = 0; g < nk; g++) {
    (*pos)[g] = static_cast<int64_t>(s.tab[3 * g]);
    (*neg)[g] = static_cast<int64_t>(s.tab[3 * g + 1]);
    (*u2)[g] = static_cast<uint64_t>(s.tab[3 * g + 2]);
  }
  return FFM_OK;
}

int ffm_engine_metrics_read_keyed(ffm_engine *e, int32_t channel, int32_t reset, ffm_keyed_metrics *out) {
  if (!out) return fail(FFM_E_INVALID, "null output");
  KeyedSnapshot s;
  if (int rc = keyed_snapshot(e, channel, reset != 0, &s)) return rc;
  std::vector<int64_t> pos, neg;
  std::vector<uint64_t> u2;
  if (int rc = keyed_columns(s, &pos, &neg, &u2)) return rc;
  if (int rc = ffm_engine_metrics_from_keyed(pos.data(), neg.data(), u2.data(), static_cast<int64_t>(pos.size()), out)) return rc;
  out->n_nan = s.n_nan;
  out->n_unkeyed = s.n_unkeyed;
  out->n_overflow = s.n_overflow;
  return FFM_OK;
}

int ffm_engine_metrics_keyed_table(ffm_engine *e, int32_t channel, int64_t cap, int32_t *key, int64_t *pos, int64_t *neg,
                                   uint64_t *u2, int64_t *n_keys) {
  if (!n_keys || cap < 0) return fail(FFM_E_INVALID, "null n_keys or negative cap");
  KeyedSnapshot s;
  if (int rc = keyed_snapshot(e, channel, false, &s)) return rc;
  const int64_t nk = static_cast<int64_t>(s.key.size());
  *n_keys = nk;
  if (nk > cap) return fail(FFM_E_CAPACITY, "the table has more keys than the arrays hold (*n_keys is set)");
  for (int64_t g = 0; g < nk; g++) {
    if (key) key[g] = s.key[g];
    if (pos) pos[g] = static_cast<int64_t>(s.tab[3 * g]);
    if (neg) neg[g] = static_cast<int64_t>(s.tab[3 * g + 1]);
    if (u2) u2[g] = static_cast<uint64_t>(s.tab[3 * g + 2]);
  }
  return FFM_OK;
}
