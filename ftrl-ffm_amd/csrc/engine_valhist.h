// engine_valhist.h -- value buckets (include/ffm_engine.h "Value buckets"), host side: a value histogram's words
// and counters in HBM, its stream and its two page-locked staging buffers, the launches of valhist_kernel
// (kernels_valhist.h); the edge rule and the host twin of the bucket step, which are host arithmetic and need no
// device; the table set on an engine.  A histogram touches nothing of an engine.  Part of engine.hip's translation
// unit (inside its extern "C" block).

struct ffm_valhist {
  int32_t n_fields = 0, device_id = 0;
  hipStream_t stream = nullptr;
  unsigned long long *d_hist = nullptr;      // [n_fields][FFM_BUCKET_BINS]
  unsigned long long *d_counters = nullptr;  // n_valid, n_bad, n_nan
  // pageable callers' entries go through one of two page-locked images, as a sketch's do (engine_sketch.h)
  ffm_sketch::Stage stage[2];
  int stage_next = 0;
};

void ffm_engine_valhist_destroy(ffm_valhist *s) {
  if (!s) return;
  (void)hipSetDevice(s->device_id);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  for (auto &st : s->stage) {
    if (st.pinned) (void)hipHostFree(st.pinned);
    if (st.ev_read) (void)hipEventDestroy(st.ev_read);
  }
  if (s->d_hist) (void)hipFree(s->d_hist);
  if (s->d_counters) (void)hipFree(s->d_counters);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
}

static int valhist_init(ffm_valhist *s) {
  HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  const size_t bytes = static_cast<size_t>(s->n_fields) * FFM_BUCKET_BINS * sizeof(unsigned long long);
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s->d_hist), bytes));
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s->d_counters), 3 * sizeof(unsigned long long)));
  HIP_TRY(hipMemsetAsync(s->d_hist, 0, bytes, s->stream));
  HIP_TRY(hipMemsetAsync(s->d_counters, 0, 3 * sizeof(unsigned long long), s->stream));
  for (auto &st : s->stage) HIP_TRY(hipEventCreateWithFlags(&st.ev_read, hipEventDisableTiming));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return FFM_OK;
}

// (a key of the kernel's cache is field << 16 | bin in 32 bits, all ones being "empty": 4096 fields = 2 GB of words)
static constexpr int32_t kValhistMaxFields = 4096;

int ffm_engine_valhist_create(int32_t n_fields, int32_t device_id, ffm_valhist **out) {
  if (!out) return fail(FFM_E_INVALID, "null output");
  *out = nullptr;
  if (n_fields <= 0 || n_fields > kValhistMaxFields) return fail(FFM_E_INVALID, "n_fields must lie in [1, 4096] (FFM only)");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
    (void)hipGetLastError();
    return fail(FFM_E_DEVICE, "no HIP device: values are counted on the GPU (there is no CPU fallback)");
  }
  if (device_id < 0 || device_id >= n_dev) return fail(FFM_E_INVALID, "device_id out of range");
  HIP_TRY(hipSetDevice(device_id));
  ffm_valhist *s = new (std::nothrow) ffm_valhist;
  if (!s) return fail(FFM_E_NOMEM, "out of host memory");
  s->n_fields = n_fields;
  s->device_id = device_id;
  if (int rc = valhist_init(s)) {
    const std::string msg = g_last_error;
    ffm_engine_valhist_destroy(s);
    return fail(rc, msg);
  }
  *out = s;
  return FFM_OK;
}

// One launch over entries the device can read: launch_sketch's grids (24 workgroups over PCIe, hash_ids_kernel's in HBM).
static void launch_valhist(ffm_valhist *s, int32_t nnz, const int32_t *field, const float *val, unsigned first, bool pcie) {
  const uintptr_t bits = reinterpret_cast<uintptr_t>(field) | reinterpret_cast<uintptr_t>(val);
  const int vec = (bits & 15u) == 0 ? 1 : 0;
  const int lanes = vec ? cdiv(nnz, 4) : nnz;
  const int grid = pcie ? 24 : std::max(1, std::min(1024, cdiv(lanes, 256)));
  const unsigned F = static_cast<unsigned>(s->n_fields);
  const unsigned *v = reinterpret_cast<const unsigned *>(val);
  if (field)
    hipLaunchKernelGGL((valhist_kernel<true>), dim3(grid), dim3(256), 0, s->stream, static_cast<unsigned>(nnz), field, v, first, F, vec,
                       s->d_hist, s->d_counters);
  else
    hipLaunchKernelGGL((valhist_kernel<false>), dim3(grid), dim3(256), 0, s->stream, static_cast<unsigned>(nnz), field, v, first, F, vec,
                       s->d_hist, s->d_counters);
}

static int valhist_args(ffm_valhist *s, int32_t nnz, const float *val) {
  if (!s) return fail(FFM_E_INVALID, "null value histogram");
  if (nnz < 0) return fail(FFM_E_INVALID, "negative nnz");
  if (nnz > 0 && !val) return fail(FFM_E_INVALID, "null value array");
  return FFM_OK;
}

int ffm_engine_valhist_add(ffm_valhist *s, int32_t nnz, const int32_t *field, const float *val, int32_t zero_copy) {
  if (int rc = valhist_args(s, nnz, val)) return rc;
  if (nnz == 0) return FFM_OK;
  HIP_TRY(hipSetDevice(s->device_id));
  if (zero_copy) {
    // the caller's page-locked arrays, read in place; back once they are read
    void *d_val = nullptr, *d_field = nullptr;
    hipError_t err = hipHostGetDevicePointer(&d_val, const_cast<float *>(val), 0);
    if (err == hipSuccess && field) err = hipHostGetDevicePointer(&d_field, const_cast<int32_t *>(field), 0);
    if (err != hipSuccess || !d_val || (field && !d_field)) {
      (void)hipGetLastError();
      return fail(FFM_E_INVALID, "zero_copy arrays must be page-locked, device-mapped host memory (ffm_engine_pin_host)");
    }
    launch_valhist(s, nnz, static_cast<const int32_t *>(d_field), static_cast<const float *>(d_val), 0u, true);
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
    std::memcpy(st.pinned, val + off, 4 * static_cast<size_t>(n));
    if (field) std::memcpy(st.pinned + half, field + off, 4 * static_cast<size_t>(n));
    void *mapped = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&mapped, st.pinned, 0));
    const char *m = static_cast<const char *>(mapped);
    launch_valhist(s, n, field ? reinterpret_cast<const int32_t *>(m + half) : nullptr, reinterpret_cast<const float *>(m),
                   static_cast<unsigned>(off), true);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(st.ev_read, s->stream));
    st.used = true;
  }
  return FFM_OK;
}

int ffm_engine_valhist_add_device(ffm_valhist *s, int32_t nnz, const int32_t *field, const float *val) {
  if (int rc = valhist_args(s, nnz, val)) return rc;
  if (nnz == 0) return FFM_OK;
  HIP_TRY(hipSetDevice(s->device_id));
  launch_valhist(s, nnz, field, val, 0u, false);
  HIP_TRY(hipGetLastError());
  return FFM_OK;
}

int ffm_engine_valhist_read(ffm_valhist *s, uint64_t *counts, int64_t *n_valid, int64_t *n_bad, int64_t *n_nan) {
  if (!s) return fail(FFM_E_INVALID, "null value histogram");
  HIP_TRY(hipSetDevice(s->device_id));
  HIP_TRY(hipStreamSynchronize(s->stream));
  unsigned long long cnt[3] = {0, 0, 0};
  HIP_TRY(hipMemcpy(cnt, s->d_counters, sizeof(cnt), hipMemcpyDeviceToHost));
  if (n_valid) *n_valid = static_cast<int64_t>(cnt[0]);
  if (n_bad) *n_bad = static_cast<int64_t>(cnt[1]);
  if (n_nan) *n_nan = static_cast<int64_t>(cnt[2]);
  if (counts)
    HIP_TRY(hipMemcpy(counts, s->d_hist, static_cast<size_t>(s->n_fields) * FFM_BUCKET_BINS * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return FFM_OK;
}

// ---- the edge rule and the bucket step on the host (no device needed) -----------------------------------------

int ffm_engine_bucket_edges(const uint64_t *counts, int32_t n_buckets, uint16_t *edges, int32_t *n_edges) {
  if (!counts || !edges || !n_edges) return fail(FFM_E_INVALID, "null array");
  if (n_buckets < 2 || n_buckets > FFM_BUCKET_MAX_EDGES + 1) return fail(FFM_E_INVALID, "n_buckets must lie in [2, 256]");
  unsigned __int128 total = 0;
  for (int b = 0; b < FFM_BUCKET_BINS; b++) total += counts[b];
  const unsigned __int128 B = static_cast<unsigned>(n_buckets);
  int32_t n = 0, j = 1;
  unsigned __int128 cum = 0;
  for (int b = 0; b < FFM_BUCKET_BINS && j < n_buckets && total != 0; b++) {
    cum += counts[b];
    // t_j = ceil(j N / B): every j whose target the cumulative count has reached has its edge here; repeats dropped
    while (j < n_buckets && cum >= (static_cast<unsigned __int128>(j) * total + B - 1) / B) {
      if (n == 0 || edges[n - 1] != b) edges[n++] = static_cast<uint16_t>(b);
      j++;
    }
  }
  *n_edges = n;
  return FFM_OK;
}

// n_edges [n_fields] (-1: not bucketed) and edges [n_fields][FFM_BUCKET_MAX_EDGES]: in range and strictly ascending.
static int bucket_table_check(int32_t n_fields, const int32_t *n_edges, const uint16_t *edges) {
  if (n_fields <= 0) return fail(FFM_E_INVALID, "value buckets need an FFM model's fields");
  if (!n_edges || !edges) return fail(FFM_E_INVALID, "null bucket table");
  for (int32_t f = 0; f < n_fields; f++) {
    if (n_edges[f] < -1 || n_edges[f] > FFM_BUCKET_MAX_EDGES)
      return fail(FFM_E_INVALID, "field " + std::to_string(f) + ": n_edges must lie in [-1, 255]");
    const uint16_t *e = edges + static_cast<size_t>(f) * FFM_BUCKET_MAX_EDGES;
    for (int32_t i = 1; i < n_edges[f]; i++)
      if (e[i] <= e[i - 1]) return fail(FFM_E_INVALID, "field " + std::to_string(f) + ": edges must be strictly ascending");
  }
  return FFM_OK;
}

int ffm_engine_bucket_ids_host(int32_t n_fields, const int32_t *n_edges, const uint16_t *edges, int32_t nnz, const int32_t *field,
                               const int32_t *feat_in, const float *val_in, int32_t *feat_out, float *val_out, uint8_t *bucketed) {
  if (int rc = bucket_table_check(n_fields, n_edges, edges)) return rc;
  if (nnz < 0) return fail(FFM_E_INVALID, "negative nnz");
  if (nnz > 0 && (!feat_in || !feat_out || !val_out)) return fail(FFM_E_INVALID, "null array");
  const ftrl_hash::Buckets bk{n_edges, edges};
  for (int32_t p = 0; p < nnz; p++) {
    int32_t ft = feat_in[p];
    uint32_t v = ftrl_hash::kOneBits;  // (val_in == NULL: the block with an array of 1.0f)
    if (val_in) std::memcpy(&v, val_in + p, 4);
    const bool hit = ftrl_hash::bucket_entry(n_fields, bk, field ? field[p] : p % n_fields, &ft, &v);
    feat_out[p] = ft;
    std::memcpy(val_out + p, &v, 4);
    if (bucketed) bucketed[p] = hit ? 1 : 0;
  }
  return FFM_OK;
}

// ---- the table on an engine --------------------------------------------------------------------------------------

// Idle as ffm_engine_set_rare_fold asks, for its reasons (engine_idcount.h): what is in flight holds the table it was
// claimed with, and is waited for before that table is freed.
int ffm_engine_set_buckets(ffm_engine *e, const int32_t *n_edges, const uint16_t *edges) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  if (!e->hash_ids) return fail(FFM_E_INVALID, "value buckets become ids that are then hashed: this engine was created without FFM_FLAG_HASH_IDS");
  if (e->m.type != FFM_MODEL_FFM) return fail(FFM_E_INVALID, "value buckets are per field: FFM engines only");
  if (e->in_group || e->m.n_shards > 1) return fail(FFM_E_UNSUPPORTED, "a group's or a shard's engine takes no bucket table");
  if (n_edges)
    if (int rc = bucket_table_check(e->m.n_fields, n_edges, edges)) return rc;
  if (e->n_staged > 0 || e->has_pending) return fail(FFM_E_INVALID, "the engine must be idle: staged blocks are still waiting");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  if (int rc = eval_launch_pending(e)) return rc;
  if (int rc = e->drain()) return rc;
  if (e->prep) HIP_TRY(hipStreamSynchronize(e->prep));
  HIP_TRY(hipStreamSynchronize(e->stream));
  ftrl_hash::Buckets next{};
  if (n_edges) {
    const size_t F = static_cast<size_t>(e->m.n_fields), head = 4 * F, body = 2 * F * FFM_BUCKET_MAX_EDGES;
    char *d = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d), head + body));
    hipError_t err = hipMemcpy(d, n_edges, head, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(d + head, edges, body, hipMemcpyHostToDevice);
    if (err != hipSuccess) {
      (void)hipFree(d);
      HIP_TRY(err);
    }
    next = ftrl_hash::Buckets{reinterpret_cast<const int32_t *>(d), reinterpret_cast<const uint16_t *>(d + head)};
  }
  if (e->buckets.n_edges) (void)hipFree(const_cast<int32_t *>(e->buckets.n_edges));
  e->buckets = next;
  return FFM_OK;
}

// For callers of the _device entry points: the engine's whole mapping (bucket, fold, hash) of a block that is
// already in HBM.  Asynchronous on the engine's stream, like ffm_engine_hash_ids_device.
int ffm_engine_bucket_ids_device(ffm_engine *e, int32_t nnz, const int32_t *field, const int32_t *feat_in, const float *val_in,
                                 int32_t *feat_out, float *val_out) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  if (nnz < 0) return fail(FFM_E_INVALID, "negative nnz");
  if (nnz > 0 && (!feat_in || !feat_out || !val_in || !val_out)) return fail(FFM_E_INVALID, "null array");
  if (!e->buckets.n_edges) return fail(FFM_E_INVALID, "this engine has no bucket table (ffm_engine_set_buckets)");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  if (int rc_e = eval_launch_pending(e)) return rc_e;
  launch_bucket_ids(e, e->stream, nnz, field, feat_in, feat_out, val_in, val_out);
  HIP_TRY(hipGetLastError());
  return FFM_OK;
}
