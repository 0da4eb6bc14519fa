// engine_valhist.h -- value buckets (include/ffm_engine.h "Value buckets"), host side: a value histogram's words
// and counters in HBM behind the counting objects' feed (engine_count.h), the launches of valhist_kernel
// (kernels_valhist.h); the edge rule and the host twin of the bucket step, which are host arithmetic and need no
// device; the table set on an engine.  A histogram touches nothing of an engine.  Part of engine.hip's translation
// unit (inside its extern "C" block).

struct ffm_valhist : CountFeed {
  int32_t n_fields = 0;
  unsigned long long *d_hist = nullptr;      // [n_fields][FFM_BUCKET_BINS]
  unsigned long long *d_counters = nullptr;  // n_valid, n_bad, n_nan
};

void ffm_engine_valhist_destroy(ffm_valhist *s) {
  if (!s) return;
  count_release(s, {s->d_hist, s->d_counters});
  delete s;
}

// (a key of the kernel's cache is field << 16 | bin in 32 bits, all ones being "empty": 4096 fields = 2 GB of words)
static constexpr int32_t kValhistMaxFields = 4096;

int ffm_engine_valhist_create(int32_t n_fields, int32_t device_id, ffm_valhist **out) {
  if (!out) return fail(FFM_E_INVALID, "null output");
  *out = nullptr;
  if (n_fields <= 0 || n_fields > kValhistMaxFields) return fail(FFM_E_INVALID, "n_fields must lie in [1, 4096] (FFM only)");
  ffm_valhist *s = nullptr;
  if (int rc = count_new(device_id, "no HIP device: values are counted on the GPU (there is no CPU fallback)", &s)) return rc;
  s->n_fields = n_fields;
  const int rc = count_init(s, {{reinterpret_cast<void **>(&s->d_hist), static_cast<size_t>(n_fields) * FFM_BUCKET_BINS * sizeof(unsigned long long)},
                                {reinterpret_cast<void **>(&s->d_counters), 3 * sizeof(unsigned long long)}});
  return count_created(s, rc, ffm_engine_valhist_destroy, out);
}

// One launch over entries the device can read (count_grid).
static void launch_valhist(ffm_valhist *s, int32_t nnz, const int32_t *field, const void *second, unsigned first, bool pcie) {
  const unsigned *v = static_cast<const unsigned *>(second);  // (the values' bits)
  const auto [vec, grid] = count_grid(nnz, field, v, pcie);
  const unsigned F = static_cast<unsigned>(s->n_fields);
  if (field)
    hipLaunchKernelGGL((valhist_kernel<true>), dim3(grid), dim3(256), 0, s->stream, static_cast<unsigned>(nnz), field, v, first, F, vec,
                       s->d_hist, s->d_counters);
  else
    hipLaunchKernelGGL((valhist_kernel<false>), dim3(grid), dim3(256), 0, s->stream, static_cast<unsigned>(nnz), field, v, first, F, vec,
                       s->d_hist, s->d_counters);
}

int ffm_engine_valhist_add(ffm_valhist *s, int32_t nnz, const int32_t *field, const float *val, int32_t zero_copy) {
  if (int rc = count_args(s, nnz, val, "null value histogram", "null value array")) return rc;
  return count_add(s, nnz, field, val, zero_copy, [s](auto... a) { launch_valhist(s, a...); });
}

int ffm_engine_valhist_add_device(ffm_valhist *s, int32_t nnz, const int32_t *field, const float *val) {
  if (int rc = count_args(s, nnz, val, "null value histogram", "null value array")) return rc;
  return count_add_device(s, nnz, field, val, [s](auto... a) { launch_valhist(s, a...); });
}

int ffm_engine_valhist_read(ffm_valhist *s, uint64_t *counts, int64_t *n_valid, int64_t *n_bad, int64_t *n_nan) {
  if (!s) return fail(FFM_E_INVALID, "null value histogram");
  if (int rc = count_read_head(s, s->d_counters, {n_valid, n_bad, n_nan})) return rc;
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

// Idle as ffm_engine_set_rare_fold asks, for its reasons (engine_idle_quiesce, engine_idcount.h).
int ffm_engine_set_buckets(ffm_engine *e, const int32_t *n_edges, const uint16_t *edges) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  if (!e->hash_ids) return fail(FFM_E_INVALID, "value buckets become ids that are then hashed: this engine was created without FFM_FLAG_HASH_IDS");
  if (e->m.type != FFM_MODEL_FFM) return fail(FFM_E_INVALID, "value buckets are per field: FFM engines only");
  if (e->in_group || e->m.n_shards > 1) return fail(FFM_E_UNSUPPORTED, "a group's or a shard's engine takes no bucket table");
  if (n_edges)
    if (int rc = bucket_table_check(e->m.n_fields, n_edges, edges)) return rc;
  if (int rc = engine_idle_quiesce(e)) return rc;
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
