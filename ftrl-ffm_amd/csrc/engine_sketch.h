// engine_sketch.h -- field sketches (include/ffm_engine.h "Field sketches"), host side: a sketch's registers and
// counters in HBM, its stream and its two page-locked staging buffers; the launches of field_sketch_kernel
// (kernels_sketch.h); the estimator and the range rule, which are host arithmetic and need no device.
// A sketch touches nothing of an engine.  Part of engine.hip's translation unit (inside its extern "C" block).

struct ffm_sketch {
  int32_t n_fields = 0, device_id = 0;
  hipStream_t stream = nullptr;
  unsigned *d_reg = nullptr;            // [n_fields][FFM_SKETCH_REGS]
  unsigned long long *d_cnt = nullptr;  // n_valid, n_bad
  // pageable callers' entries go through one of two page-locked images: feat, then field, each padded to 16 bytes
  struct Stage { char *pinned = nullptr; size_t cap = 0; hipEvent_t ev_read = nullptr; bool used = false; } stage[2];
  int stage_next = 0;
  ftrl_hash::Rare filter{};  // ffm_engine_sketch_set_filter: the keep-map in HBM (the sketch's own copy) or none
};

// Entries per launch of a call from host memory: a multiple of 4 (the kernel's `first`), 32 MB of staging at the most.
static constexpr int32_t kSketchChunk = 1 << 22;

void ffm_engine_sketch_destroy(ffm_sketch *s) {
  if (!s) return;
  (void)hipSetDevice(s->device_id);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  for (auto &st : s->stage) {
    if (st.pinned) (void)hipHostFree(st.pinned);
    if (st.ev_read) (void)hipEventDestroy(st.ev_read);
  }
  if (s->d_reg) (void)hipFree(s->d_reg);
  if (s->d_cnt) (void)hipFree(s->d_cnt);
  if (s->filter.words) (void)hipFree(const_cast<uint64_t *>(s->filter.words));
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
}

static int sketch_init(ffm_sketch *s) {
  HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  const size_t reg_bytes = static_cast<size_t>(s->n_fields) * FFM_SKETCH_REGS * sizeof(unsigned);
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s->d_reg), reg_bytes));
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s->d_cnt), 2 * sizeof(unsigned long long)));
  HIP_TRY(hipMemsetAsync(s->d_reg, 0, reg_bytes, s->stream));
  HIP_TRY(hipMemsetAsync(s->d_cnt, 0, 2 * sizeof(unsigned long long), s->stream));
  for (auto &st : s->stage) HIP_TRY(hipEventCreateWithFlags(&st.ev_read, hipEventDisableTiming));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return FFM_OK;
}

int ffm_engine_sketch_create(int32_t n_fields, int32_t device_id, ffm_sketch **out) {
  if (!out) return fail(FFM_E_INVALID, "null output");
  *out = nullptr;
  if (n_fields <= 0) return fail(FFM_E_INVALID, "n_fields must be positive");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
    (void)hipGetLastError();
    return fail(FFM_E_DEVICE, "no HIP device: a field sketch is filled on the GPU (there is no CPU fallback)");
  }
  if (device_id < 0 || device_id >= n_dev) return fail(FFM_E_INVALID, "device_id out of range");
  HIP_TRY(hipSetDevice(device_id));
  ffm_sketch *s = new (std::nothrow) ffm_sketch;
  if (!s) return fail(FFM_E_NOMEM, "out of host memory");
  s->n_fields = n_fields;
  s->device_id = device_id;
  if (int rc = sketch_init(s)) {
    const std::string msg = g_last_error;
    ffm_engine_sketch_destroy(s);
    return fail(rc, msg);
  }
  *out = s;
  return FFM_OK;
}

// One launch over entries the device can read.  pcie: they lie in host memory -- the upload's few workgroups
// (every PCIe read in flight holds an L2 miss entry); in HBM: the grid of hash_ids_kernel.
static void launch_sketch(ffm_sketch *s, int32_t nnz, const int32_t *field, const int32_t *feat, unsigned first, bool pcie) {
  const uintptr_t bits = reinterpret_cast<uintptr_t>(field) | reinterpret_cast<uintptr_t>(feat);
  const int vec = (bits & 15u) == 0 ? 1 : 0;
  const int lanes = vec ? cdiv(nnz, 4) : nnz;
  const int grid = pcie ? 24 : std::max(1, std::min(1024, cdiv(lanes, 256)));
  const unsigned F = static_cast<unsigned>(s->n_fields);
  if (s->filter.words) {
    if (field)
      hipLaunchKernelGGL((field_sketch_kernel<true, true, ftrl_hash::Rare>), dim3(grid), dim3(256), 0, s->stream,
                         static_cast<unsigned>(nnz), field, feat, first, F, vec, s->d_reg, s->d_cnt, s->filter);
    else
      hipLaunchKernelGGL((field_sketch_kernel<false, true, ftrl_hash::Rare>), dim3(grid), dim3(256), 0, s->stream,
                         static_cast<unsigned>(nnz), field, feat, first, F, vec, s->d_reg, s->d_cnt, s->filter);
  } else if (field)
    hipLaunchKernelGGL((field_sketch_kernel<true, false>), dim3(grid), dim3(256), 0, s->stream, static_cast<unsigned>(nnz), field, feat,
                       first, F, vec, s->d_reg, s->d_cnt);
  else
    hipLaunchKernelGGL((field_sketch_kernel<false, false>), dim3(grid), dim3(256), 0, s->stream, static_cast<unsigned>(nnz), field, feat,
                       first, F, vec, s->d_reg, s->d_cnt);
}

// A keep-map of 2^bits slots from host memory into an allocation of its own on the current device (engine_idcount.h
// makes such maps; an engine and a sketch each hold their copy).
static int rare_map_upload(int32_t bits, const uint64_t *words, ftrl_hash::Rare *out) {
  const size_t bytes = (static_cast<size_t>(1) << bits) / 8;
  uint64_t *d = nullptr;
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d), bytes));
  const hipError_t err = hipMemcpy(d, words, bytes, hipMemcpyHostToDevice);
  if (err != hipSuccess) {
    (void)hipFree(d);
    HIP_TRY(err);
  }
  *out = ftrl_hash::Rare{d, 32u - static_cast<uint32_t>(bits)};
  return FFM_OK;
}

int ffm_engine_sketch_set_filter(ffm_sketch *s, int32_t bits, const uint64_t *words) {
  if (!s) return fail(FFM_E_INVALID, "null sketch");
  if (words && (bits < 8 || bits > 30)) return fail(FFM_E_INVALID, "bits must lie in [8, 30]");
  HIP_TRY(hipSetDevice(s->device_id));
  HIP_TRY(hipStreamSynchronize(s->stream));  // (launches behind earlier adds still read the map they were given)
  ftrl_hash::Rare next{};
  if (words)
    if (int rc = rare_map_upload(bits, words, &next)) return rc;
  if (s->filter.words) (void)hipFree(const_cast<uint64_t *>(s->filter.words));
  s->filter = next;
  return FFM_OK;
}

static int sketch_args(ffm_sketch *s, int32_t nnz, const int32_t *feat) {
  if (!s) return fail(FFM_E_INVALID, "null sketch");
  if (nnz < 0) return fail(FFM_E_INVALID, "negative nnz");
  if (nnz > 0 && !feat) return fail(FFM_E_INVALID, "null id array");
  return FFM_OK;
}

int ffm_engine_sketch_add(ffm_sketch *s, int32_t nnz, const int32_t *field, const int32_t *feat, int32_t zero_copy) {
  if (int rc = sketch_args(s, nnz, feat)) return rc;
  if (nnz == 0) return FFM_OK;
  HIP_TRY(hipSetDevice(s->device_id));
  if (zero_copy) {
    // the caller's page-locked arrays, read in place; back once they are read
    void *d_feat = nullptr, *d_field = nullptr;
    hipError_t err = hipHostGetDevicePointer(&d_feat, const_cast<int32_t *>(feat), 0);
    if (err == hipSuccess && field) err = hipHostGetDevicePointer(&d_field, const_cast<int32_t *>(field), 0);
    if (err != hipSuccess || !d_feat || (field && !d_field)) {
      (void)hipGetLastError();
      return fail(FFM_E_INVALID, "zero_copy arrays must be page-locked, device-mapped host memory (ffm_engine_pin_host)");
    }
    launch_sketch(s, nnz, static_cast<const int32_t *>(d_field), static_cast<const int32_t *>(d_feat), 0u, true);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s->stream));
    return FFM_OK;
  }
  // pageable arrays: chunk by chunk into the staging buffer whose last launch has read it; the caller's arrays
  // are free again once the last chunk is copied, the kernels run behind
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
    launch_sketch(s, n, field ? reinterpret_cast<const int32_t *>(m + half) : nullptr, reinterpret_cast<const int32_t *>(m),
                  static_cast<unsigned>(off), true);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(st.ev_read, s->stream));
    st.used = true;
  }
  return FFM_OK;
}

int ffm_engine_sketch_add_device(ffm_sketch *s, int32_t nnz, const int32_t *field, const int32_t *feat) {
  if (int rc = sketch_args(s, nnz, feat)) return rc;
  if (nnz == 0) return FFM_OK;
  HIP_TRY(hipSetDevice(s->device_id));
  launch_sketch(s, nnz, field, feat, 0u, false);
  HIP_TRY(hipGetLastError());
  return FFM_OK;
}

int ffm_engine_sketch_read(ffm_sketch *s, uint8_t *reg, int64_t *n_valid, int64_t *n_bad) {
  if (!s) return fail(FFM_E_INVALID, "null sketch");
  HIP_TRY(hipSetDevice(s->device_id));
  HIP_TRY(hipStreamSynchronize(s->stream));
  unsigned long long cnt[2] = {0, 0};
  HIP_TRY(hipMemcpy(cnt, s->d_cnt, sizeof(cnt), hipMemcpyDeviceToHost));
  if (n_valid) *n_valid = static_cast<int64_t>(cnt[0]);
  if (n_bad) *n_bad = static_cast<int64_t>(cnt[1]);
  if (reg) {
    const size_t n = static_cast<size_t>(s->n_fields) * FFM_SKETCH_REGS;
    std::vector<unsigned> words(n);
    HIP_TRY(hipMemcpy(words.data(), s->d_reg, n * sizeof(unsigned), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) reg[i] = static_cast<uint8_t>(words[i]);
  }
  return FFM_OK;
}

// The estimator of include/ffm_engine.h "Field sketches", in double, registers in ascending index.
int ffm_engine_sketch_estimate(const uint8_t *reg, int32_t n_fields, double *distinct) {
  if (n_fields <= 0) return fail(FFM_E_INVALID, "n_fields must be positive");
  if (!reg || !distinct) return fail(FFM_E_INVALID, "null array");
  const double M = static_cast<double>(FFM_SKETCH_REGS), alpha = 0.7213 / (1.0 + 1.079 / M);
  for (int32_t f = 0; f < n_fields; f++) {
    const uint8_t *r = reg + static_cast<size_t>(f) * FFM_SKETCH_REGS;
    double sum = 0.0;
    int zeros = 0;
    for (int i = 0; i < FFM_SKETCH_REGS; i++) {
      sum += std::ldexp(1.0, -static_cast<int>(r[i]));
      zeros += r[i] == 0;
    }
    double est = alpha * M * M / sum;
    if (est <= 2.5 * M && zeros > 0) est = M * std::log(M / static_cast<double>(zeros));
    distinct[f] = zeros == FFM_SKETCH_REGS ? 0.0 : est;
  }
  return FFM_OK;
}

// The range rule of include/ffm_engine.h "Field sketches": exact integers.
int ffm_engine_field_ranges(const int64_t *count, int32_t n_fields, int32_t n_feats, int32_t *field_start) {
  if (n_fields <= 0) return fail(FFM_E_INVALID, "n_fields must be positive");
  if (!count || !field_start) return fail(FFM_E_INVALID, "null array");
  if (n_feats < 0 || static_cast<int64_t>(n_feats) < 2 * static_cast<int64_t>(n_fields))
    return fail(FFM_E_INVALID, "field ranges need n_feats >= 2 * n_fields");
  for (int32_t f = 0; f < n_fields; f++)
    if (count[f] < 0) return fail(FFM_E_INVALID, "negative count for field " + std::to_string(f));
  const uint64_t F = static_cast<uint64_t>(n_fields), N = static_cast<uint64_t>(n_feats);
  const uint64_t base = std::min<uint64_t>(4096, N / (2 * F)), R = N - F * base;
  auto clamped = [&](int32_t f) { return static_cast<uint64_t>(std::min<int64_t>(std::max<int64_t>(count[f], 1), int64_t{1} << 31)); };
  uint64_t C = 0;
  for (int32_t f = 0; f < n_fields; f++) C += clamped(f);
  std::vector<uint64_t> width(F), rem(F);
  uint64_t given = 0;
  for (int32_t f = 0; f < n_fields; f++) {
    const uint64_t prod = R * clamped(f);  // (below 2^63)
    width[f] = base + prod / C;
    rem[f] = prod % C;
    given += width[f];
  }
  std::vector<int32_t> order(F);
  for (int32_t f = 0; f < n_fields; f++) order[f] = f;
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return rem[a] > rem[b]; });  // (ties: the lower field)
  const uint64_t left = N - given;  // (below n_fields: each floor drops less than one id)
  for (uint64_t j = 0; j < left; j++) width[order[j]]++;
  uint64_t at = 0;
  for (int32_t f = 0; f < n_fields; f++) {
    field_start[f] = static_cast<int32_t>(at);
    at += width[f];
  }
  field_start[n_fields] = static_cast<int32_t>(at);
  return FFM_OK;
}
