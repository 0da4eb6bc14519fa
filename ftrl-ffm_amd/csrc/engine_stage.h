// engine_stage.h -- rows streaming from host memory inside the training loop: staging slots, the
// upload kernel, the score download kernel, stage_batch / train_staged / train_batch_async[_pinned] /
// predict_batch_async[_scores].
// Part of engine.hip's translation unit (included inside its extern "C" block).

// ---- pipelined host-buffer training ---------------------------------------------------------

// Upload of one staged block by a kernel: the five CSR arrays are read straight out of page-locked
// (device-mapped) host memory, 16 bytes per lane, and written to the staging slot's device arrays.
// A hipMemcpyAsync here makes the SUBMITTING THREAD wait until the stream's earlier kernels have
// finished (measured: mean 0.38 ms, up to 16 ms per call) -- the host then cannot run ahead of the
// GPU and every other step starts ~230 us late; a kernel launch never blocks.
// Every wave starts with a system-scope acquire (it drops the non-coherent lines of its L2): a
// caller that refills a block buffer it has used before (the trainers' ring) must not be served
// lines of the previous block that are still on-die, should the runtime map its page-locked memory
// cacheable.  (System-scope LOADS instead -- 8 bytes per lane -- halved the upload rate.)
struct PullJob {
  const char *src[5]; char *dst[5]; unsigned bytes[5];
  long long ordinal; long long *pulled; unsigned *ticket;  // completion word (host memory), see h_pulled
  // rows handed over without a field array (one entry per field in field order): the slot's field
  // array is written here -- entry j of the block is field j mod n_fields -- instead of crossing PCIe
  int *gen_field; unsigned gen_n; int gen_fields;
};
// The kernel's text, shared with the weighted variant below.  Macros on purpose: the same text as a
// `__device__ __forceinline__` function called by both kernels compiles pull_block_kernel to 48 SGPRs and 16
// VGPRs instead of 22 and 14 (the job struct, passed on by reference, is then loaded whole up front), and an
// unweighted block's upload has to stay the kernel it was (profiles/sample_weights.md).
#define FFM_PULL_BLOCK_ARRAYS(job)                                                                          \
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");                                                             \
  const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;              \
  _Pragma("unroll")                                                                                         \
  for (int a = 0; a < 5; a++) {                                                                             \
    const unsigned n16 = job.bytes[a] >> 4;                                                                 \
    const int4 *s = reinterpret_cast<const int4 *>(job.src[a]);                                             \
    int4 *d = reinterpret_cast<int4 *>(job.dst[a]);                                                         \
    /* (one load per lane in flight: two, four and eight measured the same -- 42 GB/s is what a kernel reads over PCIe here) */ \
    for (unsigned i = tid; i < n16; i += stride) d[i] = s[i];                                               \
    const unsigned tail = job.bytes[a] & 15u; /* sizes are multiples of 4 */                                \
    if (tid < (tail >> 2))                                                                                  \
      reinterpret_cast<int *>(job.dst[a])[(n16 << 2) + tid] = reinterpret_cast<const int *>(job.src[a])[(n16 << 2) + tid]; \
  }
#define FFM_PULL_BLOCK_FINISH(job)                                                                          \
  if (job.gen_n) {                                                                                          \
    const unsigned n4 = job.gen_n >> 2, F = static_cast<unsigned>(job.gen_fields);                          \
    for (unsigned i = tid; i < n4; i += stride) {                                                           \
      const unsigned f0 = (4u * i) % F, f1 = f0 + 1u < F ? f0 + 1u : 0u, f2 = f1 + 1u < F ? f1 + 1u : 0u;   \
      reinterpret_cast<int4 *>(job.gen_field)[i] = make_int4(static_cast<int>(f0), static_cast<int>(f1), static_cast<int>(f2), \
                                                             static_cast<int>(f2 + 1u < F ? f2 + 1u : 0u)); \
    }                                                                                                       \
    if (tid < (job.gen_n & 3u)) job.gen_field[(n4 << 2) + tid] = static_cast<int>(((n4 << 2) + tid) % F);   \
  }                                                                                                         \
  /* the workgroup that finishes last publishes the block's number to the host */                           \
  __syncthreads(); /* (every load of this workgroup has returned: its stores were issued after them) */     \
  if (threadIdx.x == 0) {                                                                                   \
    __threadfence();                                                                                        \
    if (atomicAdd(job.ticket, 1u) == gridDim.x - 1) {                                                       \
      *job.ticket = 0u;                                                                                     \
      __hip_atomic_store(job.pulled, job.ordinal, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);             \
    }                                                                                                       \
  }
__global__ __launch_bounds__(256) void pull_block_kernel(PullJob job) {
  FFM_PULL_BLOCK_ARRAYS(job)
  FFM_PULL_BLOCK_FINISH(job)
}
// A block with sample weights: the sixth array, n_rows floats, moves with the other five (whole 16-byte
// vectors, then the last n_rows % 4 floats as single words) -- a kernel of its own, so that an
// unweighted block's upload is the launch, and the kernel, it always was.
struct PullWeightedJob { PullJob block; const char *wsrc; char *wdst; unsigned wbytes; };
__global__ __launch_bounds__(256) void pull_block_weighted_kernel(PullWeightedJob wjob) {
  const PullJob &job = wjob.block;
  FFM_PULL_BLOCK_ARRAYS(job)
  {
    const unsigned n16 = wjob.wbytes >> 4;
    const int4 *s = reinterpret_cast<const int4 *>(wjob.wsrc);
    int4 *d = reinterpret_cast<int4 *>(wjob.wdst);
    for (unsigned i = tid; i < n16; i += stride) d[i] = s[i];
    const unsigned tail = wjob.wbytes & 15u;
    if (tid < (tail >> 2))
      reinterpret_cast<int *>(wjob.wdst)[(n16 << 2) + tid] = reinterpret_cast<const int *>(wjob.wsrc)[(n16 << 2) + tid];
  }
  FFM_PULL_BLOCK_FINISH(job)
}
// FFM_FLAG_HASH_IDS: the same two kernels with the ids hashed on their way through (csrc/hash_ids.h) --
// kernels of their own, so that an unflagged engine's upload is the launch, and the kernel, it always was.
// feat and field are taken out of the block's five arrays (their byte counts there are 0) and move in ONE
// loop instead: they are equally long, so a lane loads the int4 of feat and the int4 of field, hashes four
// entries and stores both; the last nnz % 4 entries go one by one.  No byte crosses PCIe twice, and the
// integer work hides behind the link (the kernel is bound by PCIe).  fsrc == nullptr: no field array came
// -- LR / FM, or FFM rows of one entry per field in field order, whose fields FFM_PULL_BLOCK_FINISH writes
// and this loop recomputes the same way.
struct PullHashJob {
  PullWeightedJob w;
  ftrl_hash::Map hm;
  const char *isrc, *fsrc; char *idst, *fdst; unsigned hbytes;
};
#define FFM_PULL_BLOCK_HASHED(hj)                                                                           \
  {                                                                                                         \
    const unsigned n16 = hj.hbytes >> 4, F = static_cast<unsigned>(hj.hm.n_fields);                         \
    for (unsigned i = tid; i < n16; i += stride) {                                                          \
      const int4 ft = reinterpret_cast<const int4 *>(hj.isrc)[i];                                           \
      int4 fl;                                                                                              \
      if (hj.fsrc) {                                                                                        \
        fl = reinterpret_cast<const int4 *>(hj.fsrc)[i];                                                    \
        reinterpret_cast<int4 *>(hj.fdst)[i] = fl;                                                          \
      } else fl = hj.hm.ffm ? hash_implicit_fields4(i, F) : make_int4(0, 0, 0, 0);                          \
      reinterpret_cast<int4 *>(hj.idst)[i] = hash_entries4(hj.hm, fl, ft);                                  \
    }                                                                                                       \
    if (tid < ((hj.hbytes & 15u) >> 2)) {                                                                   \
      const unsigned p = (n16 << 2) + tid;                                                                  \
      int f = hj.hm.ffm ? static_cast<int>(p % F) : 0;                                                      \
      if (hj.fsrc) {                                                                                        \
        f = reinterpret_cast<const int *>(hj.fsrc)[p];                                                      \
        reinterpret_cast<int *>(hj.fdst)[p] = f;                                                            \
      }                                                                                                     \
      reinterpret_cast<int *>(hj.idst)[p] = ftrl_hash::hash_entry(hj.hm, f, reinterpret_cast<const int *>(hj.isrc)[p]); \
    }                                                                                                       \
  }
__global__ __launch_bounds__(256) void pull_block_hashed_kernel(PullHashJob hjob) {
  const PullJob &job = hjob.w.block;
  FFM_PULL_BLOCK_ARRAYS(job)
  FFM_PULL_BLOCK_HASHED(hjob)
  FFM_PULL_BLOCK_FINISH(job)
}
__global__ __launch_bounds__(256) void pull_block_weighted_hashed_kernel(PullHashJob hjob) {
  const PullJob &job = hjob.w.block;
  FFM_PULL_BLOCK_ARRAYS(job)
  {
    const unsigned n16 = hjob.w.wbytes >> 4;
    const int4 *s = reinterpret_cast<const int4 *>(hjob.w.wsrc);
    int4 *d = reinterpret_cast<int4 *>(hjob.w.wdst);
    for (unsigned i = tid; i < n16; i += stride) d[i] = s[i];
    const unsigned tail = hjob.w.wbytes & 15u;
    if (tid < (tail >> 2))
      reinterpret_cast<int *>(hjob.w.wdst)[(n16 << 2) + tid] = reinterpret_cast<const int *>(hjob.w.wsrc)[(n16 << 2) + tid];
  }
  FFM_PULL_BLOCK_HASHED(hjob)
  FFM_PULL_BLOCK_FINISH(job)
}
// A block handed over without values (val == NULL: every value is 1.0f, include/ffm_engine.h "Rows without
// values"): nothing of val is in the job's five arrays, and the upload writes the slot's val array itself,
// over its own grid stride, the way FFM_PULL_BLOCK_FINISH writes a missing field array -- a lane stores four
// 1.0f as one 16-byte vector, the last n % 4 go singly.  The stores hide behind the link (the kernel is bound
// by PCIe).  Every such block writes them again: a block that brought its values may have used the slot in
// between.  Kernels of their own once more, so that a block WITH its values is uploaded by the launch, and
// the kernel, it always was; the four above keep their text (profiles/implicit_ones.md).
#define FFM_PULL_BLOCK_ONES(dst, n)                                                                         \
  {                                                                                                         \
    const unsigned n4 = (n) >> 2;                                                                           \
    const float4 ones4 = make_float4(1.0f, 1.0f, 1.0f, 1.0f);                                               \
    for (unsigned i = tid; i < n4; i += stride) reinterpret_cast<float4 *>(dst)[i] = ones4;                 \
    if (tid < ((n) & 3u)) (dst)[(n4 << 2) + tid] = 1.0f;                                                    \
  }
#define FFM_PULL_BLOCK_WEIGHTS(wj)                                                                          \
  {                                                                                                         \
    const unsigned n16 = wj.wbytes >> 4;                                                                    \
    const int4 *s = reinterpret_cast<const int4 *>(wj.wsrc);                                                \
    int4 *d = reinterpret_cast<int4 *>(wj.wdst);                                                            \
    for (unsigned i = tid; i < n16; i += stride) d[i] = s[i];                                               \
    const unsigned tail = wj.wbytes & 15u;                                                                  \
    if (tid < (tail >> 2))                                                                                  \
      reinterpret_cast<int *>(wj.wdst)[(n16 << 2) + tid] = reinterpret_cast<const int *>(wj.wsrc)[(n16 << 2) + tid]; \
  }
__global__ __launch_bounds__(256) void pull_block_ones_kernel(PullJob job, float *ones, unsigned n_ones) {
  FFM_PULL_BLOCK_ARRAYS(job)
  FFM_PULL_BLOCK_ONES(ones, n_ones)
  FFM_PULL_BLOCK_FINISH(job)
}
__global__ __launch_bounds__(256) void pull_block_weighted_ones_kernel(PullWeightedJob wjob, float *ones, unsigned n_ones) {
  const PullJob &job = wjob.block;
  FFM_PULL_BLOCK_ARRAYS(job)
  FFM_PULL_BLOCK_WEIGHTS(wjob)
  FFM_PULL_BLOCK_ONES(ones, n_ones)
  FFM_PULL_BLOCK_FINISH(job)
}
__global__ __launch_bounds__(256) void pull_block_hashed_ones_kernel(PullHashJob hjob, float *ones, unsigned n_ones) {
  const PullJob &job = hjob.w.block;
  FFM_PULL_BLOCK_ARRAYS(job)
  FFM_PULL_BLOCK_HASHED(hjob)
  FFM_PULL_BLOCK_ONES(ones, n_ones)
  FFM_PULL_BLOCK_FINISH(job)
}
__global__ __launch_bounds__(256) void pull_block_weighted_hashed_ones_kernel(PullHashJob hjob, float *ones, unsigned n_ones) {
  const PullJob &job = hjob.w.block;
  FFM_PULL_BLOCK_ARRAYS(job)
  FFM_PULL_BLOCK_WEIGHTS(hjob.w)
  FFM_PULL_BLOCK_HASHED(hjob)
  FFM_PULL_BLOCK_ONES(ones, n_ones)
  FFM_PULL_BLOCK_FINISH(job)
}
#undef FFM_PULL_BLOCK_WEIGHTS
#undef FFM_PULL_BLOCK_ONES
#undef FFM_PULL_BLOCK_HASHED
#undef FFM_PULL_BLOCK_ARRAYS
#undef FFM_PULL_BLOCK_FINISH

// The mirror image of the upload: the scores of one predicted block go from e->d_out to the caller's
// page-locked (device-mapped) host memory, 16 bytes per lane -- a lane carries four rows --, the last
// n % 4 floats as single stores.  A kernel for the reason pull_block_kernel is one: a hipMemcpyAsync
// makes the submitting thread wait for the stream's earlier kernels.  Launched on the MAIN stream
// right behind the block's predict kernel (eval_launch_pending), so it needs no event.
// The stores leave the device: every lane follows its own with a system-scope release fence (the
// upload's agent-scope __threadfence() orders nothing towards the host), and the workgroup that
// finishes last publishes the block's staging number into h_scored, again at system scope -- a host
// that reads the number (ffm_engine_blocks_scored, an acquire load) then reads whole scores.
// It writes n floats and nothing behind them.
struct PushJob {
  const float *src; float *dst; unsigned n;
  long long ordinal; long long *scored; unsigned *ticket;  // completion word (host memory), see h_scored
};
__global__ __launch_bounds__(256) void push_scores_kernel(PushJob job) {
  const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  const unsigned n4 = job.n >> 2;
  const float4 *s = reinterpret_cast<const float4 *>(job.src);
  float4 *d = reinterpret_cast<float4 *>(job.dst);
  for (unsigned i = tid; i < n4; i += stride) d[i] = s[i];
  if (tid < (job.n & 3u)) job.dst[(n4 << 2) + tid] = job.src[(n4 << 2) + tid];
  __threadfence_system();
  __syncthreads();  // (every wave of this workgroup is past its fence: its scores are in host memory)
  if (threadIdx.x == 0) {
    if (__hip_atomic_fetch_add(job.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
      *job.ticket = 0u;
      __hip_atomic_store(job.scored, job.ordinal, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

static int slots_init(ffm_engine *e) {
  if (e->slots_ready) return FFM_OK;
  const size_t R = static_cast<size_t>(e->max_rows), E = static_cast<size_t>(e->max_nnz);
  const size_t bytes = 4 * (R + 1) + 4 * E * 3 + 4 * R + 5 * 16;  // each of the 5 arrays is padded to 16 B
  for (auto &sl : e->slots) {
    // (portable: page-locked for EVERY device of the process -- an ffm_group's engines sit on
    // different GPUs and all read host blocks)
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&sl.pinned), bytes, hipHostMallocPortable | hipHostMallocMapped));
    int rc;
    if ((rc = e->alloc(&sl.row_ptr, R + 1)) || (rc = e->alloc(&sl.field, E)) || (rc = e->alloc(&sl.feat, E)) ||
        (rc = e->alloc(&sl.val, E)) || (rc = e->alloc(&sl.label, R)))
      return rc;
    HIP_TRY(hipEventCreateWithFlags(&sl.ev_copied, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&sl.ev_trained, hipEventDisableTiming));
  }
  HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&e->h_pulled), 64, hipHostMallocPortable | hipHostMallocMapped));
  *e->h_pulled = 0;
  HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&e->d_pulled), e->h_pulled, 0));
  if (int rc_t = e->alloc(&e->d_pull_ticket, 1)) return rc_t;
  HIP_TRY(hipMemsetAsync(e->d_pull_ticket, 0, sizeof(unsigned), e->prep));
  HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&e->h_scored), 64, hipHostMallocPortable | hipHostMallocMapped));
  *e->h_scored = 0;
  HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&e->d_scored), e->h_scored, 0));
  if (int rc_t = e->alloc(&e->d_score_ticket, 1)) return rc_t;
  HIP_TRY(hipMemsetAsync(e->d_score_ticket, 0, sizeof(unsigned), e->stream));
  int rc = e->alloc(&e->d_loss_acc, 1);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(e->d_loss_acc, 0, sizeof(double), e->stream));
  e->slots_ready = true;
  return FFM_OK;
}

// The slots' weight arrays (device) and their pinned images: made by the first weighted block.
static int slot_weights_init(ffm_engine *e) {
  if (e->slot_weights_ready) return FFM_OK;
  const size_t R = static_cast<size_t>(e->max_rows);
  for (auto &sl : e->slots) {
    if (!sl.pinned_w)
      HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&sl.pinned_w), 4 * R + 16, hipHostMallocPortable | hipHostMallocMapped));
    if (!sl.weight)
      if (int rc = e->alloc(&sl.weight, R)) return rc;
  }
  e->slot_weights_ready = true;
  return FFM_OK;
}

int ffm_engine_pin_host(void *p, size_t bytes) {
  if (!p || !bytes) return fail(FFM_E_INVALID, "null range");
  // portable: one registration serves every GPU of the process (an ffm_group stages the same host
  // block on all of its engines; without the flag only the current device may read it)
  HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterPortable | hipHostRegisterMapped));
  return FFM_OK;
}
int ffm_engine_unpin_host(void *p) {
  if (!p) return fail(FFM_E_INVALID, "null pointer");
  HIP_TRY(hipHostUnregister(p));
  return FFM_OK;
}

// The next staging slot for a host block: waits until the slot's own pinned image is free, copies
// the caller's arrays into it (unless zero_copy) and describes the upload (pull_block_kernel's
// argument; the block's ordinal is n_staged_total + 1).  Bookkeeping of the slot is the caller's.
static int claim_slot(ffm_engine *e, int32_t n_rows, int32_t nnz, const int32_t *row_ptr,
                      const int32_t *field, const int32_t *feat, const float *val, const int32_t *label,
                      int32_t zero_copy, int *slot_out, bool *was_used, PullJob *job_out,
                      const float *weight = nullptr, PullWeightedJob *wjob_out = nullptr, PullHashJob *hjob_out = nullptr) {
  int rc;
  if ((rc = slots_init(e))) return rc;
  if (weight && n_rows > 0 && (rc = slot_weights_init(e))) return rc;
  ffm_engine::Slot &sl = e->slots[e->slot_next];
  *slot_out = e->slot_next;
  *was_used = sl.used;
  if (sl.used && !sl.zero_copy) {
    ScopedTimer tm("stage:slot_wait");
    // the slot's own pinned image must have been pulled before it is overwritten.  (Not so for a
    // zero_copy block, whose image is the caller's: blocking the submitting thread here costs
    // ~0.2 ms per step; such callers ask ffm_engine_blocks_pulled before reusing their memory.)
    if ((rc = e->wait_issued(sl.seq))) return rc;
    HIP_TRY(hipEventSynchronize(sl.ev_copied));
  }
  // host arrays -> pinned image (the caller may reuse its buffers on return) -> device, prep stream
  const size_t R1 = static_cast<size_t>(n_rows) + 1, E = static_cast<size_t>(nnz);
  char *p = sl.pinned;
  PullJob &job = *job_out;
  int n_job = 0;
  // page-locked source of each array: the caller's own (zero_copy: untouched until the block has
  // trained) or its image in the slot's pinned buffer; the device then pulls it (pull_block_kernel)
  // (hashed_src: the array is feat or field of a flagged engine's block -- it goes to the hashed loop of the
  // upload kernel, *hashed_src / *hashed_dst, instead of into the job's five)
  auto put = [&](const void *src, size_t bytes, void *dst, const char **hashed_src = nullptr, char **hashed_dst = nullptr) -> hipError_t {
    if (!bytes || !src) return hipSuccess;
    const void *host = src;
    if (!zero_copy) {
      std::memcpy(p, src, bytes);
      host = p;
      p += (bytes + 15) & ~static_cast<size_t>(15);
    }
    void *mapped = nullptr;
    hipError_t err = hipHostGetDevicePointer(&mapped, const_cast<void *>(host), 0);
    if (err != hipSuccess) return err;
    if ((reinterpret_cast<uintptr_t>(mapped) & 15u) != 0) return hipErrorInvalidValue;  // 16-byte aligned arrays only
    if (hashed_src) {
      *hashed_src = static_cast<const char *>(mapped);
      *hashed_dst = static_cast<char *>(dst);
      return hipSuccess;
    }
    job.src[n_job] = static_cast<const char *>(mapped);
    job.dst[n_job] = static_cast<char *>(dst);
    job.bytes[n_job] = static_cast<unsigned>(bytes);
    n_job++;
    return hipSuccess;
  };
  PullHashJob *const hj = e->hash_ids ? hjob_out : nullptr;
  if (hj) {
    hj->hm = e->hm;
    hj->hbytes = static_cast<unsigned>(4 * E);
  }
  ScopedTimer tm("stage:copies");
  HIP_TRY(put(row_ptr, 4 * R1, sl.row_ptr));
  if (field) HIP_TRY(put(field, 4 * E, sl.field, hj ? &hj->fsrc : nullptr, hj ? &hj->fdst : nullptr));
  else if (e->m.type == FFM_MODEL_FFM && E > 0) {  // (validated: one entry per field in field order)
    job.gen_field = sl.field;
    job.gen_n = static_cast<unsigned>(E);
    job.gen_fields = e->m.n_fields;
  }
  HIP_TRY(put(feat, 4 * E, sl.feat, hj ? &hj->isrc : nullptr, hj ? &hj->idst : nullptr));
  HIP_TRY(put(val, 4 * E, sl.val));  // (val == NULL: nothing to copy or describe -- the upload kernel writes ones)
  HIP_TRY(put(label, 4 * static_cast<size_t>(n_rows), sl.label));
  if (weight && n_rows > 0) {  // the sixth array: beside the job's five (its image: the slot's pinned_w)
    const size_t wbytes = 4 * static_cast<size_t>(n_rows);
    const void *host = weight;
    if (!zero_copy) {
      std::memcpy(sl.pinned_w, weight, wbytes);
      host = sl.pinned_w;
    }
    void *mapped = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&mapped, const_cast<void *>(host), 0));
    wjob_out->wsrc = static_cast<const char *>(mapped);
    wjob_out->wdst = reinterpret_cast<char *>(sl.weight);
    wjob_out->wbytes = static_cast<unsigned>(wbytes);
  }
  job.ordinal = e->n_staged_total + 1;
  job.pulled = e->d_pulled;
  job.ticket = e->d_pull_ticket;
  return FFM_OK;
}

// Stage one block of host rows: (pinned image ->) HBM -> grouping, all on the prep stream.
int ffm_engine_stage_batch_weighted(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr,
                                    const int32_t *field, const int32_t *feat, const float *val,
                                    const int32_t *label, const float *weight, int32_t zero_copy) {
  SERVE_REFUSE(e, "training");  // (staging is training's: prediction stages through predict_batch_async)
  int32_t nnz = 0;
  int longest = 1;
  // (LR / FM rows have no fields -- libsvm: src/data/parser.cpp:20 gives every entry field 0 -- so a
  // field array the caller passes along is not uploaded: a third of the block's bytes over PCIe)
  if (e && e->m.type != FFM_MODEL_FFM) field = nullptr;
  int rc = validate_host_block(e, n_rows, row_ptr, field, feat, val, &nnz, &longest, true);
  if (rc) return rc;
  const bool has_field = field != nullptr || (e->m.type == FFM_MODEL_FFM && nnz > 0);  // (uploaded or written by the upload kernel)
  if (n_rows > 0 && !label) return fail(FFM_E_INVALID, "training needs labels");
  if (n_rows == 0) weight = nullptr;
  if (weight) {  // refused here, on the caller's thread, before anything of the block is queued
    if ((rc = validate_host_weights(n_rows, weight))) return rc;
    if (zero_copy) {
      if ((reinterpret_cast<uintptr_t>(weight) & 15u) != 0) return fail(FFM_E_INVALID, "a zero_copy weight array must be 16-byte aligned");
      void *mapped = nullptr;
      if (hipHostGetDevicePointer(&mapped, const_cast<float *>(weight), 0) != hipSuccess || !mapped) {
        (void)hipGetLastError();
        return fail(FFM_E_INVALID, "a zero_copy weight array must be page-locked, device-mapped host memory (ffm_engine_pin_host)");
      }
      if ((reinterpret_cast<uintptr_t>(mapped) & 15u) != 0) return fail(FFM_E_INVALID, "a zero_copy weight array must be 16-byte aligned");
    }
  }
  if ((rc = eval_launch_pending(e))) return rc;
  if (e->n_staged >= ffm_engine::kSlots - 1) return fail(FFM_E_CAPACITY, "three staged blocks are already waiting");
  if (e->has_pending) return fail(FFM_E_INVALID, "stage between train_forward and train_update");
  // everything ffm_engine_prepare_device can refuse is refused HERE, before the upload kernel is
  // launched: that kernel publishes the block's ordinal to ffm_engine_blocks_pulled, and a block
  // that then failed to stage would leave the count one ahead for good
  if (e->n_prepared >= ffm_engine::kSets - 1) return fail(FFM_E_CAPACITY, "three prepared blocks are already waiting");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  int this_slot = 0;
  bool slot_was_used = false;
  PullHashJob hjob{};  // (the hashed loop's part is filled on a flagged engine only)
  PullWeightedJob &job = hjob.w;
  if ((rc = claim_slot(e, n_rows, nnz, row_ptr, field, feat, val, label, zero_copy, &this_slot, &slot_was_used, &job.block,
                       weight, &job, &hjob)))
    return rc;
  ffm_engine::Slot &sl = e->slots[this_slot];
  // its grouping, behind its own upload on the prep stream: planned here, submitted with the upload
  PrepPlan plan;
  if ((rc = prepare_plan(e, Rows{n_rows, nnz, sl.row_ptr, has_field ? sl.field : nullptr, sl.feat, sl.val, nullptr}, &plan)))
    return rc;
  const int64_t seq = e->n_staged_total + 1;
  const int grid_pull = e->grid_pull;
  const bool timed = e->prof_on;  // (then submit runs the job on this thread)
  hipEvent_t free_ev = slot_was_used ? sl.free_ev : nullptr;
  const bool hashed = e->hash_ids;
  // (val == NULL: the upload writes the slot's values -- every time, whatever the slot held before)
  float *const ones = sl.val;
  const unsigned n_ones = val ? 0u : static_cast<unsigned>(nnz);
  rc = e->submit([e, this_slot, free_ev, hjob, hashed, plan, seq, grid_pull, timed, ones, n_ones]() -> int {
    const PullWeightedJob &job = hjob.w;
    ScopedTimer tm("stage:submit");
    ffm_engine::Slot &s2 = e->slots[this_slot];
    int rc2 = FFM_OK;
    auto body = [&]() -> int {
      HIP_TRY(hipSetDevice(e->cfg.device_id));
      if (free_ev) HIP_TRY(hipStreamWaitEvent(e->prep, free_ev, 0));  // nothing reads its device arrays
      // (long steps: the upload too waits for the running block's row kernel to end -- beside the update
      // launches it costs nothing, beside the row kernel, which is bound by the bytes it moves, it does)
      if (e->pull_after_row && plan.ws >= 0) HIP_TRY(hipStreamWaitEvent(e->prep, e->prep_after_row ? e->ev_row_done[plan.ws] : e->ev_set_free[plan.ws], 0));
      if (n_ones) {
        if (hashed && job.wbytes) hipLaunchKernelGGL(pull_block_weighted_hashed_ones_kernel, dim3(grid_pull), dim3(256), 0, e->prep, hjob, ones, n_ones);
        else if (hashed) hipLaunchKernelGGL(pull_block_hashed_ones_kernel, dim3(grid_pull), dim3(256), 0, e->prep, hjob, ones, n_ones);
        else if (job.wbytes) hipLaunchKernelGGL(pull_block_weighted_ones_kernel, dim3(grid_pull), dim3(256), 0, e->prep, job, ones, n_ones);
        else hipLaunchKernelGGL(pull_block_ones_kernel, dim3(grid_pull), dim3(256), 0, e->prep, job.block, ones, n_ones);
      }
      else if (hashed && job.wbytes) hipLaunchKernelGGL(pull_block_weighted_hashed_kernel, dim3(grid_pull), dim3(256), 0, e->prep, hjob);
      else if (hashed) hipLaunchKernelGGL(pull_block_hashed_kernel, dim3(grid_pull), dim3(256), 0, e->prep, hjob);
      else if (job.wbytes) hipLaunchKernelGGL(pull_block_weighted_kernel, dim3(grid_pull), dim3(256), 0, e->prep, job);
      else hipLaunchKernelGGL(pull_block_kernel, dim3(grid_pull), dim3(256), 0, e->prep, job.block);
      HIP_TRY(hipEventRecord(s2.ev_copied, e->prep));
      return prepare_submit(e, plan, timed);
    };
    rc2 = body();
    {
      std::lock_guard<std::mutex> lock(e->wmu);
      e->staged_issued = seq;  // (also after a failure: nobody may wait for it forever)
    }
    return rc2;
  });
  if (rc) return rc;
  sl.used = true;
  sl.zero_copy = zero_copy != 0;
  sl.n_rows = n_rows;
  sl.nnz = nnz;
  sl.row_cap = longest;
  sl.has_field = has_field;
  sl.has_weight = weight != nullptr;
  sl.seq = ++e->n_staged_total;
  e->slot_next = (e->slot_next + 1) % ffm_engine::kSlots;
  e->staged[e->n_staged++] = this_slot;
  return FFM_OK;
}
int ffm_engine_stage_batch(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr,
                           const int32_t *field, const int32_t *feat, const float *val,
                           const int32_t *label, int32_t zero_copy) {
  return ffm_engine_stage_batch_weighted(e, n_rows, row_ptr, field, feat, val, label, nullptr, zero_copy);
}

// How many of the blocks staged so far have been uploaded (their host arrays are free again).
int64_t ffm_engine_blocks_pulled(ffm_engine *e) {
  if (!e || !e->slots_ready) return 0;
  e->n_pulled = std::max<int64_t>(e->n_pulled, __atomic_load_n(e->h_pulled, __ATOMIC_ACQUIRE));
  return e->n_pulled;
}

// The staging number of the last block whose scores are whole in the caller's buffer.  (Scored
// blocks finish in staging order on the main stream; the max only keeps a second reader of a
// number it has already seen from ever getting less.)
int64_t ffm_engine_blocks_scored(ffm_engine *e) {
  if (!e || !e->slots_ready) return 0;
  const int64_t seen = __atomic_load_n(e->h_scored, __ATOMIC_ACQUIRE);
  int64_t had = __atomic_load_n(&e->n_scored, __ATOMIC_RELAXED);
  while (seen > had && !__atomic_compare_exchange_n(&e->n_scored, &had, seen, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
  return std::max(seen, had);
}

// Phase 1 (grouping is done: refresh + forward) on the oldest staged block.
int ffm_engine_train_forward_staged(ffm_engine *e, float *partial_logit) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  SERVE_REFUSE(e, "training");
  if (e->n_staged == 0) return fail(FFM_E_INVALID, "no staged block");
  if (e->has_pending) return fail(FFM_E_INVALID, "the previous block still awaits train_update");
  const int slot = e->staged[0];
  ffm_engine::Slot &sl = e->slots[slot];
  e->staged_row_cap = sl.row_cap;
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  if (int rc_w = e->wait_issued(sl.seq)) return rc_w;  // its upload + grouping launches are out
  // its grouping (behind the upload on the prep stream, or waiting for it there) implies the upload:
  // the main stream waits for ev_copied itself only when that grouping was discarded
  const Rows staged_rows{sl.n_rows, sl.nnz, sl.row_ptr, sl.has_field ? sl.field : nullptr, sl.feat, sl.val, nullptr};
  if (!(e->n_prepared > 0 && same_block(e->prepared_rows[0], staged_rows)))
    HIP_TRY(hipStreamWaitEvent(e->stream, sl.ev_copied, 0));
  int rc = train_forward_core(e, sl.n_rows, sl.nnz, sl.row_ptr, sl.has_field ? sl.field : nullptr,
                              sl.feat, sl.val, sl.label, sl.has_weight ? sl.weight : nullptr, partial_logit);
  if (rc) return rc;
  for (int i = 1; i < e->n_staged; i++) e->staged[i - 1] = e->staged[i];
  e->n_staged--;
  e->cur_slot = slot;  // released (ev_trained) by the train_update that follows
  return FFM_OK;
}

// Whole step (ffm_engine_train_batch_device) on the oldest staged block.
int ffm_engine_train_staged(ffm_engine *e, float *logit_out, double *loss_sum_out) {
  if (e && e->m.n_shards > 1)
    return fail(FFM_E_INVALID, "sharded engines train with train_forward_staged + all-reduce + train_update");
  if (e) { e->whole_step = true; e->own_logit_out = logit_out; }
  int rc = ffm_engine_train_forward_staged(e, nullptr);
  if (e) e->whole_step = false;
  if (rc) return rc;
  return ffm_engine_train_update_device(e, nullptr, logit_out, loss_sum_out);
}

// ... with its loss going into the running sum of the flush.
static int train_one_staged(ffm_engine *e) {
  int rc = ffm_engine_train_staged(e, nullptr, e->d_loss_sum);
  if (rc) return rc;
  hipLaunchKernelGGL(loss_accumulate_kernel, dim3(1), dim3(1), 0, e->stream, e->d_loss_acc, e->d_loss_sum);
  return FFM_OK;
}

// zero_copy == 0: train what the previous call staged; the block staged just now keeps uploading and
// grouping beside it (and beside the caller's preparation of the next one).  zero_copy != 0: block t+2
// is staged: train block t (bench.py's schedule; the grouping of t+2 then has its window beside
// block t and until block t+1 ends)
int ffm_engine_train_batch_async_weighted(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr,
                                          const int32_t *field, const int32_t *feat, const float *val,
                                          const int32_t *label, const float *weight, int32_t zero_copy) {
  if (e && e->m.n_shards > 1)
    return fail(FFM_E_INVALID, "sharded engines train with stage_batch + train_forward_staged + all-reduce + train_update");
  int rc = ffm_engine_stage_batch_weighted(e, n_rows, row_ptr, field, feat, val, label, weight, zero_copy ? 1 : 0);
  if (rc) return rc;
  const int keep = zero_copy ? 2 : 1;
  while (e->n_staged > keep)
    if ((rc = train_one_staged(e))) return rc;
  return FFM_OK;
}

int ffm_engine_train_batch_async(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr,
                                 const int32_t *field, const int32_t *feat, const float *val,
                                 const int32_t *label) {
  return ffm_engine_train_batch_async_weighted(e, n_rows, row_ptr, field, feat, val, label, nullptr, 0);
}

int ffm_engine_train_batch_async_pinned(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr,
                                        const int32_t *field, const int32_t *feat, const float *val,
                                        const int32_t *label) {
  return ffm_engine_train_batch_async_weighted(e, n_rows, row_ptr, field, feat, val, label, nullptr, 1);
}

// The predict launch of the block ffm_engine_predict_batch_async uploaded one call ago,
// and the download of its scores where the caller gave a buffer for them.
static int eval_launch_pending(ffm_engine *e) {
  if (!e->eval_pending.on) return FFM_OK;
  e->eval_pending.on = false;  // (first: the launch below passes check_block)
  ffm_engine::Slot &sl = e->slots[e->eval_pending.slot];
  const bool labelled = e->eval_pending.labelled;
  float *const scores = e->eval_pending.scores;
  const int output_prob = e->eval_pending.output_prob;
  const int64_t seq = e->eval_pending.seq;
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  auto launch = [&]() -> int {
    HIP_TRY(hipStreamWaitEvent(e->stream, sl.ev_copied, 0));
    e->staged_row_cap = sl.row_cap;
    int rc = ffm_engine_predict_batch_device(e, sl.n_rows, sl.nnz, sl.row_ptr, sl.has_field ? sl.field : nullptr, sl.feat,
                                             sl.val, labelled ? sl.label : nullptr, output_prob, e->d_out,
                                             labelled ? e->d_loss_sum : nullptr);
    if (rc) return rc;
    if (labelled) hipLaunchKernelGGL(loss_accumulate_kernel, dim3(1), dim3(1), 0, e->stream, e->d_loss_acc, e->d_loss_sum);
    if (scores) {
      // the block's scores to the caller's buffer, behind its predict kernel on the same stream
      // (a block without rows still publishes its number, in order)
      const PushJob job{e->d_out, scores, static_cast<unsigned>(sl.n_rows), static_cast<long long>(seq), e->d_scored, e->d_score_ticket};
      const int grid = std::max(1, std::min(e->grid_push, cdiv(sl.n_rows >> 2, 256)));
      LAUNCH(e, K_PUSH_SCORES, push_scores_kernel, grid, 256, 0, job);
    }
    HIP_TRY(hipGetLastError());
    return FFM_OK;
  };
  const int rc = launch();
  // (also after a failure: the slot's device arrays are free again -- nothing else will ever say so)
  const hipError_t err_ev = hipEventRecord(sl.ev_trained, e->stream);
  sl.free_ev = sl.ev_trained;
  if (rc) return fail(rc, "deferred predict_batch_async block " + std::to_string(seq) + ": " + g_last_error);
  HIP_TRY(err_ev);
  return FFM_OK;
}

// Pipelined evaluation: upload through a staging slot on the side stream, predict on the main one.
// The predict launch of a block is DEFERRED by one call (the caller reads nothing before
// ffm_engine_train_flush): call t submits the upload of block t and then the predict of block t-1, so
// that the upload kernel -- 24 workgroups that must find room on the chip -- is in its queue BEFORE
// the predict kernel that fills every wave slot, not behind it (round 5: 51.9 M rows/s with the H2D
// against 68.6 M resident).  The deferred launch is made by the next call of any entry point that
// puts work on the main stream (check_block), by ffm_engine_sync / check_errors and by the flush.
// scores_host (may be NULL): the block's predictions also go to the caller's page-locked buffer
// (push_scores_kernel, behind the deferred predict launch).
int ffm_engine_predict_batch_async_scores(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr,
                                          const int32_t *field, const int32_t *feat, const float *val,
                                          const int32_t *label, int32_t zero_copy, int32_t output_prob,
                                          float *scores_host) {
  int32_t nnz = 0;
  int longest = 1;
  if (e && e->m.type != FFM_MODEL_FFM) field = nullptr;  // (LR / FM: no fields to upload)
  if (e) e->eval_hold = true;  // (the deferred block waits until this one's upload is submitted)
  int rc = validate_host_block(e, n_rows, row_ptr, field, feat, val, &nnz, &longest, true);
  if (e) e->eval_hold = false;
  if (rc) return rc;
  const bool has_field = field != nullptr || (e->m.type == FFM_MODEL_FFM && nnz > 0);  // (uploaded or written by the upload kernel)
  if (e->m.n_shards > 1) return fail(FFM_E_INVALID, "a sharded engine predicts through predict_batch_device + predict_finish_device");
  if (e->n_staged > 0 || e->has_pending) return fail(FFM_E_INVALID, "staged training blocks are still waiting");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  // (refused before the upload is launched: that kernel publishes the block's number)
  float *scores_dev = nullptr;
  if (scores_host) {
    if ((reinterpret_cast<uintptr_t>(scores_host) & 15u) != 0) return fail(FFM_E_INVALID, "scores_host must be 16-byte aligned");
    void *mapped = nullptr;
    if (hipHostGetDevicePointer(&mapped, scores_host, 0) != hipSuccess || !mapped) {
      (void)hipGetLastError();
      return fail(FFM_E_INVALID, "scores_host must be page-locked, device-mapped host memory (ffm_engine_pin_host)");
    }
    if ((reinterpret_cast<uintptr_t>(mapped) & 15u) != 0) return fail(FFM_E_INVALID, "scores_host must be 16-byte aligned");
    scores_dev = static_cast<float *>(mapped);
  }
  if ((rc = e->drain())) return rc;
  int this_slot = 0;
  bool slot_was_used = false;
  PullHashJob hjob{};  // (the hashed loop's part is filled on a flagged engine only)
  PullJob &job = hjob.w.block;
  if ((rc = claim_slot(e, n_rows, nnz, row_ptr, field, feat, val, label, zero_copy, &this_slot, &slot_was_used, &job, nullptr,
                       nullptr, &hjob)))
    return rc;
  ffm_engine::Slot &sl = e->slots[this_slot];
  if (slot_was_used && sl.free_ev) HIP_TRY(hipStreamWaitEvent(e->prep, sl.free_ev, 0));  // nothing reads its device arrays
  if (!val && nnz > 0) {  // (no values came: the upload writes the slot's)
    if (e->hash_ids) hipLaunchKernelGGL(pull_block_hashed_ones_kernel, dim3(e->grid_pull), dim3(256), 0, e->prep, hjob, sl.val, static_cast<unsigned>(nnz));
    else hipLaunchKernelGGL(pull_block_ones_kernel, dim3(e->grid_pull), dim3(256), 0, e->prep, job, sl.val, static_cast<unsigned>(nnz));
  }
  else if (e->hash_ids) hipLaunchKernelGGL(pull_block_hashed_kernel, dim3(e->grid_pull), dim3(256), 0, e->prep, hjob);
  else hipLaunchKernelGGL(pull_block_kernel, dim3(e->grid_pull), dim3(256), 0, e->prep, job);
  HIP_TRY(hipEventRecord(sl.ev_copied, e->prep));
  sl.used = true;
  sl.zero_copy = zero_copy != 0;
  sl.n_rows = n_rows;
  sl.nnz = nnz;
  sl.row_cap = longest;
  sl.has_field = has_field;
  sl.seq = ++e->n_staged_total;
  {
    std::lock_guard<std::mutex> lock(e->wmu);
    e->staged_issued = sl.seq;
  }
  e->slot_next = (e->slot_next + 1) % ffm_engine::kSlots;
  HIP_TRY(hipGetLastError());
  if ((rc = eval_launch_pending(e))) return rc;  // the block of the call before, behind this upload
  e->eval_pending.on = true;
  e->eval_pending.slot = this_slot;
  e->eval_pending.labelled = label != nullptr;
  e->eval_pending.scores = scores_dev;
  e->eval_pending.output_prob = scores_dev ? (output_prob != 0) : 0;
  e->eval_pending.seq = sl.seq;
  if (e->eval_defer_off) return eval_launch_pending(e);  // (FFM_EVAL_DEFER=0: as rounds 3-5)
  return FFM_OK;
}

int ffm_engine_predict_batch_async(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr,
                                   const int32_t *field, const int32_t *feat, const float *val,
                                   const int32_t *label, int32_t zero_copy) {
  return ffm_engine_predict_batch_async_scores(e, n_rows, row_ptr, field, feat, val, label, zero_copy, 0, nullptr);
}

int ffm_engine_train_flush(ffm_engine *e, double *loss_sum_out) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  int rc;
  if ((rc = eval_launch_pending(e))) return rc;
  if (e->m.n_shards == 1)
    while (e->n_staged > 0)
      if ((rc = train_one_staged(e))) return rc;
  double total = 0.0;
  if (e->slots_ready) {
    HIP_TRY(hipMemcpyAsync(&total, e->d_loss_acc, sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemsetAsync(e->d_loss_acc, 0, sizeof(double), e->stream));
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (loss_sum_out) *loss_sum_out = total;
  return check_device_errors(e);
}
