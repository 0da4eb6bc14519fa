// engine_count.h -- what the counting objects share (field sketches, engine_sketch.h; rare ids, engine_idcount.h;
// value buckets, engine_valhist.h), host side: the feed -- a stream and two page-locked staging images -- with the
// loop that takes a caller's arrays through it, the launch geometry, and the common steps of create, add and read.
// Each object keeps its arrays, its kernel launch and its arithmetic.  Part of engine.hip's translation unit
// (in front of its extern "C" block: the helpers are templates).

// Every counting object is a feed with arrays of its own behind it.
struct CountFeed {
  int32_t device_id = 0;
  hipStream_t stream = nullptr;
  // pageable callers' entries go through one of two page-locked images: the second array (feat or val), then field,
  // each padded to 16 bytes
  struct Stage { char *pinned = nullptr; size_t cap = 0; hipEvent_t ev_read = nullptr; bool used = false; } stage[2];
  int stage_next = 0;
};

// Entries per launch of a call from host memory: a multiple of 4 (the kernels' `first`), 32 MB of staging at the most.
static constexpr int32_t kCountChunk = 1 << 22;

struct CountArray { void **ptr; size_t bytes; };

// The stream, the object's arrays in HBM (zeroed) and the two events.
static int count_init(CountFeed *f, std::initializer_list<CountArray> arrays) {
  HIP_TRY(hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking));
  for (const CountArray &a : arrays) {
    HIP_TRY(hipMalloc(a.ptr, a.bytes));
    HIP_TRY(hipMemsetAsync(*a.ptr, 0, a.bytes, f->stream));
  }
  for (auto &st : f->stage) HIP_TRY(hipEventCreateWithFlags(&st.ev_read, hipEventDisableTiming));
  HIP_TRY(hipStreamSynchronize(f->stream));
  return FFM_OK;
}

// What count_init made, or as much of it as there is: waits for the stream first.
static void count_release(CountFeed *f, std::initializer_list<const void *> arrays) {
  (void)hipSetDevice(f->device_id);
  if (f->stream) (void)hipStreamSynchronize(f->stream);
  for (auto &st : f->stage) {
    if (st.pinned) (void)hipHostFree(st.pinned);
    if (st.ev_read) (void)hipEventDestroy(st.ev_read);
  }
  for (const void *a : arrays)
    if (a) (void)hipFree(const_cast<void *>(a));
  if (f->stream) (void)hipStreamDestroy(f->stream);
}

// The head of a create: the device chosen and a fresh object on it.  no_device: the caller's FFM_E_DEVICE message.
template <class T>
static int count_new(int32_t device_id, const char *no_device, T **s) {
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
    (void)hipGetLastError();
    return fail(FFM_E_DEVICE, no_device);
  }
  if (device_id < 0 || device_id >= n_dev) return fail(FFM_E_INVALID, "device_id out of range");
  HIP_TRY(hipSetDevice(device_id));
  *s = new (std::nothrow) T;
  if (!*s) return fail(FFM_E_NOMEM, "out of host memory");
  (*s)->device_id = device_id;
  return FFM_OK;
}

// The tail of a create: rc is the object's init; a failure keeps its message across the destroy.
template <class T>
static int count_created(T *s, int rc, void (*destroy)(T *), T **out) {
  if (rc) {
    const std::string msg = g_last_error;
    destroy(s);
    return fail(rc, msg);
  }
  *out = s;
  return FFM_OK;
}

static int count_args(const CountFeed *f, int32_t nnz, const void *second, const char *null_handle, const char *null_array) {
  if (!f) return fail(FFM_E_INVALID, null_handle);
  if (nnz < 0) return fail(FFM_E_INVALID, "negative nnz");
  if (nnz > 0 && !second) return fail(FFM_E_INVALID, null_array);
  return FFM_OK;
}

// The geometry of one launch over entries the device can read.  vec: both arrays are 16-byte aligned, a lane takes
// four entries.  pcie: they lie in host memory -- the upload's few workgroups (every PCIe read in flight holds an L2
// miss entry); in HBM: the grid of hash_ids_kernel.
struct CountGrid { int vec, grid; };
static CountGrid count_grid(int32_t nnz, const void *field, const void *second, bool pcie) {
  const uintptr_t bits = reinterpret_cast<uintptr_t>(field) | reinterpret_cast<uintptr_t>(second);
  const int vec = (bits & 15u) == 0 ? 1 : 0;
  const int lanes = vec ? cdiv(nnz, 4) : nnz;
  return {vec, pcie ? 24 : std::max(1, std::min(1024, cdiv(lanes, 256)))};
}

// The entries of a call from host memory.  field may be null; second is feat or val (4-byte elements either way).
// launch(n, d_field, d_second, first, pcie) makes the object's launch on f->stream over n entries the device can
// read, the call's entries from `first` on.
template <class Launch>
static int count_add(CountFeed *f, int32_t nnz, const int32_t *field, const void *second, int32_t zero_copy, Launch launch) {
  if (nnz == 0) return FFM_OK;
  HIP_TRY(hipSetDevice(f->device_id));
  if (zero_copy) {
    // the caller's page-locked arrays, read in place; back once they are read
    void *d_second = nullptr, *d_field = nullptr;
    hipError_t err = hipHostGetDevicePointer(&d_second, const_cast<void *>(second), 0);
    if (err == hipSuccess && field) err = hipHostGetDevicePointer(&d_field, const_cast<int32_t *>(field), 0);
    if (err != hipSuccess || !d_second || (field && !d_field)) {
      (void)hipGetLastError();
      return fail(FFM_E_INVALID, "zero_copy arrays must be page-locked, device-mapped host memory (ffm_engine_pin_host)");
    }
    launch(nnz, static_cast<const int32_t *>(d_field), static_cast<const void *>(d_second), 0u, true);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(f->stream));
    return FFM_OK;
  }
  // pageable arrays: chunk by chunk into the staging buffer whose last launch has read it; the caller's arrays
  // are free again once the last chunk is copied, the kernels run behind
  const char *from = static_cast<const char *>(second);
  for (int32_t off = 0; off < nnz; off += kCountChunk) {
    const int32_t n = std::min(kCountChunk, nnz - off);
    const size_t half = (4 * static_cast<size_t>(n) + 15) & ~static_cast<size_t>(15), need = field ? 2 * half : half;
    CountFeed::Stage &st = f->stage[f->stage_next];
    f->stage_next ^= 1;
    if (st.used) HIP_TRY(hipEventSynchronize(st.ev_read));
    if (st.cap < need) {
      if (st.pinned) HIP_TRY(hipHostFree(st.pinned));
      st.pinned = nullptr;
      st.cap = 0;
      HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&st.pinned), need, hipHostMallocPortable | hipHostMallocMapped));
      st.cap = need;
    }
    std::memcpy(st.pinned, from + 4 * static_cast<size_t>(off), 4 * static_cast<size_t>(n));
    if (field) std::memcpy(st.pinned + half, field + off, 4 * static_cast<size_t>(n));
    void *mapped = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&mapped, st.pinned, 0));
    const char *m = static_cast<const char *>(mapped);
    launch(n, field ? reinterpret_cast<const int32_t *>(m + half) : nullptr, static_cast<const void *>(m), static_cast<unsigned>(off), true);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(st.ev_read, f->stream));
    st.used = true;
  }
  return FFM_OK;
}

// The same for arrays in device memory: one launch, asynchronous.
template <class Launch>
static int count_add_device(CountFeed *f, int32_t nnz, const int32_t *field, const void *second, Launch launch) {
  if (nnz == 0) return FFM_OK;
  HIP_TRY(hipSetDevice(f->device_id));
  launch(nnz, field, second, 0u, false);
  HIP_TRY(hipGetLastError());
  return FFM_OK;
}

// The head of a read: everything added so far has been counted, and the object's first counters are in *out[i]
// (where that is not null).
static int count_read_head(CountFeed *f, const unsigned long long *d_counters, std::initializer_list<int64_t *> out) {
  HIP_TRY(hipSetDevice(f->device_id));
  HIP_TRY(hipStreamSynchronize(f->stream));
  unsigned long long cnt[3] = {0, 0, 0};
  HIP_TRY(hipMemcpy(cnt, d_counters, out.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  size_t i = 0;
  for (int64_t *o : out) {
    if (o) *o = static_cast<int64_t>(cnt[i]);
    i++;
  }
  return FFM_OK;
}
