// engine_sketch.h -- field sketches (include/ffm_engine.h "Field sketches"), host side: a sketch's registers and
// counters in HBM behind the counting objects' feed (engine_count.h); the launches of field_sketch_kernel
// (kernels_sketch.h); the estimator and the range rule, which are host arithmetic and need no device.
// A sketch touches nothing of an engine.  Part of engine.hip's translation unit (inside its extern "C" block).

struct ffm_sketch : CountFeed {
  int32_t n_fields = 0;
  unsigned *d_reg = nullptr;            // [n_fields][FFM_SKETCH_REGS]
  unsigned long long *d_cnt = nullptr;  // n_valid, n_bad
  ftrl_hash::Rare filter{};  // ffm_engine_sketch_set_filter: the keep-map in HBM (the sketch's own copy) or none
};

void ffm_engine_sketch_destroy(ffm_sketch *s) {
  if (!s) return;
  count_release(s, {s->d_reg, s->d_cnt, s->filter.words});
  delete s;
}

int ffm_engine_sketch_create(int32_t n_fields, int32_t device_id, ffm_sketch **out) {
  if (!out) return fail(FFM_E_INVALID, "null output");
  *out = nullptr;
  if (n_fields <= 0) return fail(FFM_E_INVALID, "n_fields must be positive");
  ffm_sketch *s = nullptr;
  if (int rc = count_new(device_id, "no HIP device: a field sketch is filled on the GPU (there is no CPU fallback)", &s)) return rc;
  s->n_fields = n_fields;
  const int rc = count_init(s, {{reinterpret_cast<void **>(&s->d_reg), static_cast<size_t>(n_fields) * FFM_SKETCH_REGS * sizeof(unsigned)},
                                {reinterpret_cast<void **>(&s->d_cnt), 2 * sizeof(unsigned long long)}});
  return count_created(s, rc, ffm_engine_sketch_destroy, out);
}

// One launch over entries the device can read (count_grid).
static void launch_sketch(ffm_sketch *s, int32_t nnz, const int32_t *field, const void *second, unsigned first, bool pcie) {
  const int32_t *feat = static_cast<const int32_t *>(second);
  const auto [vec, grid] = count_grid(nnz, field, feat, pcie);
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

int ffm_engine_sketch_add(ffm_sketch *s, int32_t nnz, const int32_t *field, const int32_t *feat, int32_t zero_copy) {
  if (int rc = count_args(s, nnz, feat, "null sketch", "null id array")) return rc;
  return count_add(s, nnz, field, feat, zero_copy, [s](auto... a) { launch_sketch(s, a...); });
}

int ffm_engine_sketch_add_device(ffm_sketch *s, int32_t nnz, const int32_t *field, const int32_t *feat) {
  if (int rc = count_args(s, nnz, feat, "null sketch", "null id array")) return rc;
  return count_add_device(s, nnz, field, feat, [s](auto... a) { launch_sketch(s, a...); });
}

int ffm_engine_sketch_read(ffm_sketch *s, uint8_t *reg, int64_t *n_valid, int64_t *n_bad) {
  if (!s) return fail(FFM_E_INVALID, "null sketch");
  if (int rc = count_read_head(s, s->d_cnt, {n_valid, n_bad})) return rc;
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
