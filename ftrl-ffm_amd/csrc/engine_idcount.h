// engine_idcount.h -- rare ids (include/ffm_engine.h "Rare ids"), host side: an id counter's words and counters in
// HBM behind the counting objects' feed (engine_count.h), the launches of idcount_kernel and of
// idcount_keep_kernel (kernels_idcount.h); the fold set on an engine; the host twin of the fold.
// A counter touches nothing of an engine.  Part of engine.hip's translation unit (inside its extern "C" block).

struct ffm_idcount : CountFeed {
  int32_t n_fields = 0, bits = 0, cap = 0;
  unsigned *d_cnt = nullptr;               // [2^bits]
  unsigned long long *d_counters = nullptr;  // n_valid, n_bad, then the keep kernel's two sums
  unsigned long long *d_words = nullptr;   // [2^bits / 64], made by the first ffm_engine_idcount_keep
};

void ffm_engine_idcount_destroy(ffm_idcount *s) {
  if (!s) return;
  count_release(s, {s->d_cnt, s->d_counters, s->d_words});
  delete s;
}

int ffm_engine_idcount_create(int32_t n_fields, int32_t bits, int32_t cap, int32_t device_id, ffm_idcount **out) {
  if (!out) return fail(FFM_E_INVALID, "null output");
  *out = nullptr;
  if (n_fields < 0) return fail(FFM_E_INVALID, "n_fields must not be negative (0: LR / FM)");
  if (bits < 8 || bits > 30) return fail(FFM_E_INVALID, "bits must lie in [8, 30]");
  if (cap < 1 || cap > 65535) return fail(FFM_E_INVALID, "cap must lie in [1, 65535]");
  ffm_idcount *s = nullptr;
  if (int rc = count_new(device_id, "no HIP device: ids are counted on the GPU (there is no CPU fallback)", &s)) return rc;
  s->n_fields = n_fields;
  s->bits = bits;
  s->cap = cap;
  const int rc = count_init(s, {{reinterpret_cast<void **>(&s->d_cnt), (static_cast<size_t>(1) << bits) * sizeof(unsigned)},
                                {reinterpret_cast<void **>(&s->d_counters), 4 * sizeof(unsigned long long)}});
  return count_created(s, rc, ffm_engine_idcount_destroy, out);
}

// One launch over entries the device can read (count_grid).
static void launch_idcount(ffm_idcount *s, int32_t nnz, const int32_t *field, const void *second, unsigned first, bool pcie) {
  if (s->n_fields == 0) field = nullptr;  // (LR / FM: the field is taken as 0)
  const int32_t *feat = static_cast<const int32_t *>(second);
  const auto [vec, grid] = count_grid(nnz, field, feat, pcie);
  const unsigned F = static_cast<unsigned>(s->n_fields), shift = 32u - static_cast<unsigned>(s->bits);
  if (field)
    hipLaunchKernelGGL((idcount_kernel<true>), dim3(grid), dim3(256), 0, s->stream, static_cast<unsigned>(nnz), field, feat, first, F,
                       vec, shift, static_cast<unsigned>(s->cap), s->d_cnt, s->d_counters);
  else
    hipLaunchKernelGGL((idcount_kernel<false>), dim3(grid), dim3(256), 0, s->stream, static_cast<unsigned>(nnz), field, feat, first, F,
                       vec, shift, static_cast<unsigned>(s->cap), s->d_cnt, s->d_counters);
}

int ffm_engine_idcount_add(ffm_idcount *s, int32_t nnz, const int32_t *field, const int32_t *feat, int32_t zero_copy) {
  if (int rc = count_args(s, nnz, feat, "null id counter", "null id array")) return rc;
  if (s->n_fields == 0) field = nullptr;  // (neither mapped nor staged)
  return count_add(s, nnz, field, feat, zero_copy, [s](auto... a) { launch_idcount(s, a...); });
}

int ffm_engine_idcount_add_device(ffm_idcount *s, int32_t nnz, const int32_t *field, const int32_t *feat) {
  if (int rc = count_args(s, nnz, feat, "null id counter", "null id array")) return rc;
  return count_add_device(s, nnz, field, feat, [s](auto... a) { launch_idcount(s, a...); });
}

int ffm_engine_idcount_read(ffm_idcount *s, uint32_t *counts, int64_t *n_valid, int64_t *n_bad) {
  if (!s) return fail(FFM_E_INVALID, "null id counter");
  if (int rc = count_read_head(s, s->d_counters, {n_valid, n_bad})) return rc;
  if (counts) {
    const size_t n = static_cast<size_t>(1) << s->bits;
    HIP_TRY(hipMemcpy(counts, s->d_cnt, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    const uint32_t cap = static_cast<uint32_t>(s->cap);
    for (size_t i = 0; i < n; i++) counts[i] = std::min(counts[i], cap);  // (a word may run past the cap: kernels_idcount.h)
  }
  return FFM_OK;
}

int ffm_engine_idcount_keep(ffm_idcount *s, int32_t min_count, uint64_t *words, int64_t *n_kept_slots, int64_t *n_folded_entries) {
  if (!s) return fail(FFM_E_INVALID, "null id counter");
  if (min_count < 1 || min_count > s->cap) return fail(FFM_E_INVALID, "min_count must lie in [1, cap]: counts above the cap are not known");
  if (!words) return fail(FFM_E_INVALID, "null output");
  HIP_TRY(hipSetDevice(s->device_id));
  const unsigned n_slots = 1u << s->bits;
  const size_t bytes = static_cast<size_t>(n_slots) / 8;
  if (!s->d_words) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s->d_words), bytes));
  HIP_TRY(hipMemsetAsync(s->d_counters + 2, 0, 2 * sizeof(unsigned long long), s->stream));
  hipLaunchKernelGGL(idcount_keep_kernel, dim3(std::max(1, std::min(1024, cdiv(static_cast<int>(n_slots), 256)))), dim3(256), 0, s->stream,
                     s->d_cnt, n_slots, static_cast<unsigned>(min_count), static_cast<unsigned>(s->cap), s->d_words, s->d_counters + 2);
  HIP_TRY(hipGetLastError());
  unsigned long long sums[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(words, s->d_words, bytes, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(sums, s->d_counters + 2, sizeof(sums), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (n_kept_slots) *n_kept_slots = static_cast<int64_t>(sums[0]);
  if (n_folded_entries) *n_folded_entries = static_cast<int64_t>(sums[1]);
  return FFM_OK;
}

// ---- the fold on an engine ---------------------------------------------------------------------------------

// Idle: no staged block waits to be trained (n_staged), none stands between train_forward and train_update
// (has_pending) -- both the engine's own bookkeeping on the caller's thread.  What is left in flight holds the map
// or the table it was claimed with (a deferred predict_batch_async block, uploads the staging thread has yet to
// issue): the deferred launch is made, the staging thread drained and both streams waited for before the old one
// is freed.  (ffm_engine_set_rare_fold, and ffm_engine_set_buckets in engine_valhist.h.)
static int engine_idle_quiesce(ffm_engine *e) {
  if (e->n_staged > 0 || e->has_pending) return fail(FFM_E_INVALID, "the engine must be idle: staged blocks are still waiting");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  if (int rc = eval_launch_pending(e)) return rc;
  if (int rc = e->drain()) return rc;
  if (e->prep) HIP_TRY(hipStreamSynchronize(e->prep));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return FFM_OK;
}

int ffm_engine_set_rare_fold(ffm_engine *e, int32_t bits, const uint64_t *words) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  if (!e->hash_ids) return fail(FFM_E_INVALID, "a rare-id fold works on raw ids: this engine was created without FFM_FLAG_HASH_IDS");
  if (e->in_group || e->m.n_shards > 1) return fail(FFM_E_UNSUPPORTED, "a group's or a shard's engine takes no rare-id fold");
  if (words && (bits < 8 || bits > 30)) return fail(FFM_E_INVALID, "bits must lie in [8, 30]");
  if (int rc = engine_idle_quiesce(e)) return rc;
  ftrl_hash::Rare next{};
  if (words)
    if (int rc = rare_map_upload(bits, words, &next)) return rc;
  if (e->rare.words) (void)hipFree(const_cast<uint64_t *>(e->rare.words));
  e->rare = next;
  return FFM_OK;
}

// The fold on the host (no device needed): the device's bits (csrc/hash_ids.h).  n_fields == 0: LR / FM.
int ffm_engine_fold_ids_host(int32_t n_fields, int32_t bits, const uint64_t *words, int32_t nnz, const int32_t *field,
                             const int32_t *feat_in, int32_t *feat_out) {
  if (n_fields < 0) return fail(FFM_E_INVALID, "n_fields must not be negative (0: LR / FM)");
  if (bits < 8 || bits > 30) return fail(FFM_E_INVALID, "bits must lie in [8, 30]");
  if (!words) return fail(FFM_E_INVALID, "null map");
  if (nnz < 0) return fail(FFM_E_INVALID, "negative nnz");
  if (nnz > 0 && (!feat_in || !feat_out)) return fail(FFM_E_INVALID, "null id array");
  const bool ffm = n_fields > 0;
  const ftrl_hash::Rare rare{words, 32u - static_cast<uint32_t>(bits)};
  for (int32_t p = 0; p < nnz; p++)
    feat_out[p] = ftrl_hash::fold_entry(ffm, n_fields, rare, !ffm ? 0 : field ? field[p] : p % n_fields, feat_in[p]);
  return FFM_OK;
}

// The slot of an entry (no device needed): what the counter counts and the map tests.
int ffm_engine_rare_slots_host(int32_t bits, int32_t nnz, const int32_t *field, const int32_t *feat, uint32_t *slot) {
  if (bits < 8 || bits > 30) return fail(FFM_E_INVALID, "bits must lie in [8, 30]");
  if (nnz < 0) return fail(FFM_E_INVALID, "negative nnz");
  if (nnz > 0 && (!feat || !slot)) return fail(FFM_E_INVALID, "null array");
  for (int32_t p = 0; p < nnz; p++) slot[p] = ftrl_hash::hash_bits(field ? field[p] : 0, feat[p]) >> (32 - bits);
  return FFM_OK;
}
