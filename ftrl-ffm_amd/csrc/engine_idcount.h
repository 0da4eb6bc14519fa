// engine_idcount.h -- rare ids (include/ffm_engine.h "Rare ids"), host side: an id counter's words and counters in
// HBM, its stream and its two page-locked staging buffers, the launches of idcount_kernel and of
// idcount_keep_kernel (kernels_idcount.h); the fold set on an engine; the host twin of the fold.
// A counter touches nothing of an engine.  Part of engine.hip's translation unit (inside its extern "C" block).

struct ffm_idcount {
  int32_t n_fields = 0, bits = 0, cap = 0, device_id = 0;
  hipStream_t stream = nullptr;
  unsigned *d_cnt = nullptr;               // [2^bits]
  unsigned long long *d_counters = nullptr;  // n_valid, n_bad, then the keep kernel's two sums
  unsigned long long *d_words = nullptr;   // [2^bits / 64], made by the first ffm_engine_idcount_keep
  // pageable callers' entries go through one of two page-locked images, as a sketch's do (engine_sketch.h)
  ffm_sketch::Stage stage[2];
  int stage_next = 0;
};

void ffm_engine_idcount_destroy(ffm_idcount *s) {
  if (!s) return;
  (void)hipSetDevice(s->device_id);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  for (auto &st : s->stage) {
    if (st.pinned) (void)hipHostFree(st.pinned);
    if (st.ev_read) (void)hipEventDestroy(st.ev_read);
  }
  if (s->d_cnt) (void)hipFree(s->d_cnt);
  if (s->d_counters) (void)hipFree(s->d_counters);
  if (s->d_words) (void)hipFree(s->d_words);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
}

static int idcount_init(ffm_idcount *s) {
  HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  const size_t bytes = (static_cast<size_t>(1) << s->bits) * sizeof(unsigned);
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s->d_cnt), bytes));
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s->d_counters), 4 * sizeof(unsigned long long)));
  HIP_TRY(hipMemsetAsync(s->d_cnt, 0, bytes, s->stream));
  HIP_TRY(hipMemsetAsync(s->d_counters, 0, 4 * sizeof(unsigned long long), s->stream));
  for (auto &st : s->stage) HIP_TRY(hipEventCreateWithFlags(&st.ev_read, hipEventDisableTiming));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return FFM_OK;
}

int ffm_engine_idcount_create(int32_t n_fields, int32_t bits, int32_t cap, int32_t device_id, ffm_idcount **out) {
  if (!out) return fail(FFM_E_INVALID, "null output");
  *out = nullptr;
  if (n_fields < 0) return fail(FFM_E_INVALID, "n_fields must not be negative (0: LR / FM)");
  if (bits < 8 || bits > 30) return fail(FFM_E_INVALID, "bits must lie in [8, 30]");
  if (cap < 1 || cap > 65535) return fail(FFM_E_INVALID, "cap must lie in [1, 65535]");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
    (void)hipGetLastError();
    return fail(FFM_E_DEVICE, "no HIP device: ids are counted on the GPU (there is no CPU fallback)");
  }
  if (device_id < 0 || device_id >= n_dev) return fail(FFM_E_INVALID, "device_id out of range");
  HIP_TRY(hipSetDevice(device_id));
  ffm_idcount *s = new (std::nothrow) ffm_idcount;
  if (!s) return fail(FFM_E_NOMEM, "out of host memory");
  s->n_fields = n_fields;
  s->bits = bits;
  s->cap = cap;
  s->device_id = device_id;
  if (int rc = idcount_init(s)) {
    const std::string msg = g_last_error;
    ffm_engine_idcount_destroy(s);
    return fail(rc, msg);
  }
  *out = s;
  return FFM_OK;
}

// One launch over entries the device can read: launch_sketch's grids (24 workgroups over PCIe, hash_ids_kernel's in HBM).
static void launch_idcount(ffm_idcount *s, int32_t nnz, const int32_t *field, const int32_t *feat, unsigned first, bool pcie) {
  if (s->n_fields == 0) field = nullptr;  // (LR / FM: the field is taken as 0)
  const uintptr_t bits = reinterpret_cast<uintptr_t>(field) | reinterpret_cast<uintptr_t>(feat);
  const int vec = (bits & 15u) == 0 ? 1 : 0;
  const int lanes = vec ? cdiv(nnz, 4) : nnz;
  const int grid = pcie ? 24 : std::max(1, std::min(1024, cdiv(lanes, 256)));
  const unsigned F = static_cast<unsigned>(s->n_fields), shift = 32u - static_cast<unsigned>(s->bits);
  if (field)
    hipLaunchKernelGGL((idcount_kernel<true>), dim3(grid), dim3(256), 0, s->stream, static_cast<unsigned>(nnz), field, feat, first, F,
                       vec, shift, static_cast<unsigned>(s->cap), s->d_cnt, s->d_counters);
  else
    hipLaunchKernelGGL((idcount_kernel<false>), dim3(grid), dim3(256), 0, s->stream, static_cast<unsigned>(nnz), field, feat, first, F,
                       vec, shift, static_cast<unsigned>(s->cap), s->d_cnt, s->d_counters);
}

static int idcount_args(ffm_idcount *s, int32_t nnz, const int32_t *feat) {
  if (!s) return fail(FFM_E_INVALID, "null id counter");
  if (nnz < 0) return fail(FFM_E_INVALID, "negative nnz");
  if (nnz > 0 && !feat) return fail(FFM_E_INVALID, "null id array");
  return FFM_OK;
}

int ffm_engine_idcount_add(ffm_idcount *s, int32_t nnz, const int32_t *field, const int32_t *feat, int32_t zero_copy) {
  if (int rc = idcount_args(s, nnz, feat)) return rc;
  if (nnz == 0) return FFM_OK;
  HIP_TRY(hipSetDevice(s->device_id));
  if (s->n_fields == 0) field = nullptr;
  if (zero_copy) {
    // the caller's page-locked arrays, read in place; back once they are read
    void *d_feat = nullptr, *d_field = nullptr;
    hipError_t err = hipHostGetDevicePointer(&d_feat, const_cast<int32_t *>(feat), 0);
    if (err == hipSuccess && field) err = hipHostGetDevicePointer(&d_field, const_cast<int32_t *>(field), 0);
    if (err != hipSuccess || !d_feat || (field && !d_field)) {
      (void)hipGetLastError();
      return fail(FFM_E_INVALID, "zero_copy arrays must be page-locked, device-mapped host memory (ffm_engine_pin_host)");
    }
    launch_idcount(s, nnz, static_cast<const int32_t *>(d_field), static_cast<const int32_t *>(d_feat), 0u, true);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s->stream));
    return FFM_OK;
  }
  // pageable arrays: chunk by chunk into the staging buffer whose last launch has read it (ffm_engine_sketch_add)
  for (int32_t off = 0; off < nnz; off += kSketchChunk) {
    const int32_t n = std::min(kSketchChunk, nnz - off);
    const size_t half = (4 * static_cast<size_t>(n) + 15) & ~static_cast<size_t>(15), need = field ? 2 * half : half;
    ffm_sketch::Stage &st = s->stage[s->stage_next];
    s->stage_next ^= 1;
    if (st.used) HIP_TRY(hipEventSynchronize(st.ev_read));
    if (st.cap < need) {
      if (st.pinned) HIP_TRY(hipHostFree(st.pinned));
      st.pinned = nullptr;
      st.cap = 0;
      HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&st.pinned), need, hipHostMallocPortable | hipHostMallocMapped));
      st.cap = need;
    }
    std::memcpy(st.pinned, feat + off, 4 * static_cast<size_t>(n));
    if (field) std::memcpy(st.pinned + half, field + off, 4 * static_cast<size_t>(n));
    void *mapped = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&mapped, st.pinned, 0));
    const char *m = static_cast<const char *>(mapped);
    launch_idcount(s, n, field ? reinterpret_cast<const int32_t *>(m + half) : nullptr, reinterpret_cast<const int32_t *>(m),
                   static_cast<unsigned>(off), true);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(st.ev_read, s->stream));
    st.used = true;
  }
  return FFM_OK;
}

int ffm_engine_idcount_add_device(ffm_idcount *s, int32_t nnz, const int32_t *field, const int32_t *feat) {
  if (int rc = idcount_args(s, nnz, feat)) return rc;
  if (nnz == 0) return FFM_OK;
  HIP_TRY(hipSetDevice(s->device_id));
  launch_idcount(s, nnz, field, feat, 0u, false);
  HIP_TRY(hipGetLastError());
  return FFM_OK;
}

int ffm_engine_idcount_read(ffm_idcount *s, uint32_t *counts, int64_t *n_valid, int64_t *n_bad) {
  if (!s) return fail(FFM_E_INVALID, "null id counter");
  HIP_TRY(hipSetDevice(s->device_id));
  HIP_TRY(hipStreamSynchronize(s->stream));
  unsigned long long cnt[2] = {0, 0};
  HIP_TRY(hipMemcpy(cnt, s->d_counters, sizeof(cnt), hipMemcpyDeviceToHost));
  if (n_valid) *n_valid = static_cast<int64_t>(cnt[0]);
  if (n_bad) *n_bad = static_cast<int64_t>(cnt[1]);
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
// it was claimed with (a deferred predict_batch_async block, uploads the staging thread has yet to issue): the
// deferred launch is made, the staging thread drained and both streams waited for before the old map is freed.
int ffm_engine_set_rare_fold(ffm_engine *e, int32_t bits, const uint64_t *words) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  if (!e->hash_ids) return fail(FFM_E_INVALID, "a rare-id fold works on raw ids: this engine was created without FFM_FLAG_HASH_IDS");
  if (e->in_group || e->m.n_shards > 1) return fail(FFM_E_UNSUPPORTED, "a group's or a shard's engine takes no rare-id fold");
  if (words && (bits < 8 || bits > 30)) return fail(FFM_E_INVALID, "bits must lie in [8, 30]");
  if (e->n_staged > 0 || e->has_pending) return fail(FFM_E_INVALID, "the engine must be idle: staged blocks are still waiting");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  if (int rc = eval_launch_pending(e)) return rc;
  if (int rc = e->drain()) return rc;
  if (e->prep) HIP_TRY(hipStreamSynchronize(e->prep));
  HIP_TRY(hipStreamSynchronize(e->stream));
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
