// engine_stage.h -- rows streaming from host memory inside the training loop, host side: the staging slots,
// the launches of the upload and score download kernels (kernels_stage.h), stage_batch / train_staged /
// train_batch_async[_pinned] / predict_batch_async[_scores].
// Part of engine.hip's translation unit (included inside its extern "C" block).

// ---- pipelined host-buffer training ---------------------------------------------------------

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

// The device's address of host memory that the 16-byte lanes of the upload and download kernels can move:
// page-locked, device-mapped and 16-byte aligned.  Null where it is not, and *why says what is wrong: the
// runtime's error (not page-locked), or hipSuccess for memory that is only not aligned.
static void *mapped16(const void *host, hipError_t *why) {
  *why = hipSuccess;
  if ((reinterpret_cast<uintptr_t>(host) & 15u) != 0) return nullptr;
  void *mapped = nullptr;
  *why = hipHostGetDevicePointer(&mapped, const_cast<void *>(host), 0);
  if (*why == hipSuccess && !mapped) *why = hipErrorInvalidValue;
  if (*why != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return (reinterpret_cast<uintptr_t>(mapped) & 15u) == 0 ? mapped : nullptr;
}
// ... for an array of the caller's own: refused (FFM_E_INVALID, last error set) where it is null.
static void *mapped16_or_refuse(const void *host, const char *what) {
  hipError_t why;
  void *mapped = mapped16(host, &why);
  if (!mapped)
    fail(FFM_E_INVALID, std::string(what) + (why == hipSuccess ? " must be 16-byte aligned"
                                                               : " must be page-locked, device-mapped host memory (ffm_engine_pin_host)"));
  return mapped;
}

// What claim_slot hands back: the slot, whether it held a block before, whether the slot's field array will
// hold the block's fields (uploaded, or written by the upload kernel), and the upload's argument -- the
// whole PullHashJob, of which an instantiation takes the part it needs (launch_upload).
struct SlotClaim {
  int slot = 0;
  bool was_used = false, has_field = false;
  PullHashJob job{};  // (the hashed loop's part is filled on a flagged engine only)
  ftrl_hash::Rare rare{};  // the engine's keep-map when the block was claimed (words == nullptr: none)
  // the engine's bucket table when the block was claimed (bk.n_edges == nullptr: none), and where val moves then
  PullBucketPart bucket{};
};

// The next staging slot for a host block (`host`: the caller's arrays, field == nullptr on LR / FM): waits
// until the slot's own pinned image is free, copies the caller's arrays into it (unless zero_copy) and
// describes the upload (the block's ordinal is n_staged_total + 1).  Bookkeeping of the slot is the
// caller's: slot_commit.
// resident (with zero_copy): the arrays of `host` are DEVICE addresses, 16-byte aligned (a closed block of a row cutter,
// engine_rows.h) -- the upload then reads HBM, and nothing is asked about host memory.
static int claim_slot(ffm_engine *e, const Rows &host, const float *weight, int32_t zero_copy, SlotClaim *claim, bool resident = false) {
  const auto [n_rows, nnz, row_ptr, field, feat, val, label] = host;
  int rc;
  if ((rc = slots_init(e))) return rc;
  if (weight && n_rows > 0 && (rc = slot_weights_init(e))) return rc;
  ffm_engine::Slot &sl = e->slots[e->slot_next];
  claim->slot = e->slot_next;
  claim->was_used = sl.used;
  if (sl.used && !sl.zero_copy) {
    ScopedTimer tm("stage:slot_wait");
    // the slot's own pinned image must have been pulled before it is overwritten.  (Not so for a
    // zero_copy block, whose image is the caller's: blocking the submitting thread here costs
    // ~0.2 ms per step; such callers ask ffm_engine_blocks_pulled before reusing their memory.)
    if ((rc = e->wait_issued(sl.seq))) return rc;
    HIP_TRY(hipEventSynchronize(sl.ev_copied));
  }
  // host arrays -> pinned image (the caller may reuse its buffers on return) -> device, prep stream
  const size_t R1 = static_cast<size_t>(n_rows) + 1, E = static_cast<size_t>(nnz), R = static_cast<size_t>(n_rows);
  char *p = sl.pinned, *pw = sl.pinned_w;
  PullHashJob &hj = claim->job;
  PullJob &job = hj.w.block;
  int n_job = 0;
  // Where put describes an array: as the next of the job's five, or as a part of the job of its own.
  struct Part { const char **src; char **dst; unsigned *bytes; };
  // page-locked source of each array: the caller's own (zero_copy: untouched until the block has
  // trained) or its image in the slot's pinned buffer (*image, which moves on); the device then pulls it
  // (pull_block_kernel)
  auto put = [&](const void *src, size_t bytes, void *dst, const Part *own = nullptr, char **image = nullptr) -> hipError_t {
    if (!bytes || !src) return hipSuccess;
    const void *host_src = src;
    if (!zero_copy) {
      char *&at = image ? *image : p;
      std::memcpy(at, src, bytes);
      host_src = at;
      at += (bytes + 15) & ~static_cast<size_t>(15);
    }
    hipError_t why = hipSuccess;
    void *mapped = resident ? const_cast<void *>(host_src) : mapped16(host_src, &why);
    if (!mapped) return why != hipSuccess ? why : hipErrorInvalidValue;  // 16-byte aligned arrays only
    const Part next{&job.src[n_job], &job.dst[n_job], &job.bytes[n_job]};
    const Part &to = own ? *own : next;
    *to.src = static_cast<const char *>(mapped);
    *to.dst = static_cast<char *>(dst);
    *to.bytes = static_cast<unsigned>(bytes);
    if (!own) n_job++;
    return hipSuccess;
  };
  // a flagged engine: feat and field go to the hashed loop of the upload kernel instead of into the job's five
  const Part hashed_ids{&hj.isrc, &hj.idst, &hj.hbytes}, hashed_fields{&hj.fsrc, &hj.fdst, &hj.hbytes};
  // the sixth array: beside the job's five (its image: the slot's pinned_w)
  const Part weights{&hj.w.wsrc, &hj.w.wdst, &hj.w.wbytes};
  if (e->hash_ids) hj.hm = e->hm;
  claim->rare = e->rare;
  // a bucket table (flagged FFM engines only): val too goes to the hashed loop, which writes all of the slot's val
  const bool bucketed = e->hash_ids && e->buckets.n_edges;
  unsigned vbytes = 0;
  const Part bucketed_vals{&claim->bucket.vsrc, &claim->bucket.vdst, &vbytes};
  if (bucketed) {
    claim->bucket.bk = e->buckets;
    claim->bucket.vdst = reinterpret_cast<char *>(sl.val);
  }
  ScopedTimer tm("stage:copies");
  HIP_TRY(put(row_ptr, 4 * R1, sl.row_ptr));
  if (field) HIP_TRY(put(field, 4 * E, sl.field, e->hash_ids ? &hashed_fields : nullptr));
  else if (e->m.type == FFM_MODEL_FFM && E > 0) {  // (validated: one entry per field in field order)
    job.gen_field = sl.field;
    job.gen_n = static_cast<unsigned>(E);
    job.gen_fields = e->m.n_fields;
  }
  claim->has_field = field != nullptr || job.gen_n != 0;
  HIP_TRY(put(feat, 4 * E, sl.feat, e->hash_ids ? &hashed_ids : nullptr));
  HIP_TRY(put(val, 4 * E, sl.val, bucketed ? &bucketed_vals : nullptr));  // (val == NULL: nothing to copy or describe -- the upload kernel writes ones)
  HIP_TRY(put(label, 4 * R, sl.label));
  HIP_TRY(put(weight, 4 * R, sl.weight, &weights, &pw));
  job.ordinal = e->n_staged_total + 1;
  job.pulled = e->d_pulled;
  job.ticket = e->d_pull_ticket;
  return FFM_OK;
}

// The upload of one claimed block on stream `st`: the one place that names an instantiation of the upload kernel.
// ones / n_ones: the slot's val array and how many 1.0f the kernel writes there (0: the block brought its values).
// rare: the claim's keep-map (set on a flagged engine only, ffm_engine_set_rare_fold); none: the launches below it.
// bucket: the claim's bucket table and val's own part (ffm_engine_set_buckets); those launches write val themselves.
static void launch_upload(ffm_engine *e, hipStream_t st, int grid, const PullHashJob &hj, const ftrl_hash::Rare &rare,
                          const PullBucketPart &bucket, float *ones, unsigned n_ones) {
  // (an engine with FFM_FLAG_NORM_ROWS, while profiling is on -- submissions then all come from the caller's thread --,
  // times it as "pull_block_kernel", the figure to read normalize_rows_kernel's next to; on every other engine the
  // upload carries no label, as always)
  struct Timed {
    ffm_engine *e; hipStream_t st;
    Timed(ffm_engine *e_, hipStream_t st_) : e(e_->prof_on && e_->norm_rows_on ? e_ : nullptr), st(st_) { if (e) e->prof_begin(K_UPLOAD, st); }
    ~Timed() { if (e) e->prof_end(st); }
  } timed(e, st);
  auto launch = [&](auto weighted, auto hashed, auto folded, const auto &arg) {
    constexpr bool W = decltype(weighted)::value, H = decltype(hashed)::value, R = decltype(folded)::value;
    if (n_ones) hipLaunchKernelGGL((pull_block_kernel<W, H, R, false, float *, unsigned>), dim3(grid), dim3(256), 0, st, arg, ones, n_ones);
    else hipLaunchKernelGGL((pull_block_kernel<W, H, R, false>), dim3(grid), dim3(256), 0, st, arg);
  };
  const std::true_type yes{};
  const std::false_type no{};
  if (e->hash_ids && bucket.bk.n_edges) {
    const PullBucketJob bj{PullRareJob{hj, rare}, bucket};
    if (hj.w.wbytes) hipLaunchKernelGGL((pull_block_kernel<true, true, false, true>), dim3(grid), dim3(256), 0, st, bj);
    else hipLaunchKernelGGL((pull_block_kernel<false, true, false, true>), dim3(grid), dim3(256), 0, st, bj);
  } else if (e->hash_ids && rare.words) {
    const PullRareJob rj{hj, rare};
    if (hj.w.wbytes) launch(yes, yes, yes, rj);
    else launch(no, yes, yes, rj);
  } else if (e->hash_ids && hj.w.wbytes) launch(yes, yes, no, hj);
  else if (e->hash_ids) launch(no, yes, no, hj);
  else if (hj.w.wbytes) launch(yes, no, no, hj.w);
  else launch(no, no, no, hj.w.block);
}

// The claimed slot holds the block from here on (its upload is submitted): number seq = n_staged_total + 1.
static void slot_commit(ffm_engine *e, const SlotClaim &claim, const Rows &host, int row_cap, bool has_weight, int32_t zero_copy) {
  ffm_engine::Slot &sl = e->slots[claim.slot];
  sl.used = true;
  sl.zero_copy = zero_copy != 0;
  sl.n_rows = host.n_rows;
  sl.nnz = host.nnz;
  sl.row_cap = row_cap;
  sl.has_field = claim.has_field;
  sl.has_weight = has_weight;
  sl.seq = ++e->n_staged_total;
  e->slot_next = (e->slot_next + 1) % ffm_engine::kSlots;
}
// The block a slot holds, as the kernels take it.
static Rows slot_rows(const ffm_engine::Slot &sl, const int *label) {
  return Rows{sl.n_rows, sl.nnz, sl.row_ptr, sl.has_field ? sl.field : nullptr, sl.feat, sl.val, label};
}

// Stage one block of host rows: (pinned image ->) HBM -> grouping, all on the prep stream.
// ... of a validated block `host` (its longest row: `longest`), from eval_launch_pending on.  resident: `host` lies
// in HBM (claim_slot) and is whole once `ready` (may be null) has happened: the upload waits for it on the prep stream.
static int stage_block_from(ffm_engine *e, const Rows &host, int longest, const float *weight, int32_t zero_copy, bool resident = false,
                            hipEvent_t ready = nullptr) {
  const auto [n_rows, nnz, row_ptr, field, feat, val, label] = host;
  int rc;
  if ((rc = eval_launch_pending(e))) return rc;
  if (e->n_staged >= ffm_engine::kSlots - 1) return fail(FFM_E_CAPACITY, "three staged blocks are already waiting");
  if (e->has_pending) return fail(FFM_E_INVALID, "stage between train_forward and train_update");
  // everything ffm_engine_prepare_device can refuse is refused HERE, before the upload kernel is
  // launched: that kernel publishes the block's ordinal to ffm_engine_blocks_pulled, and a block
  // that then failed to stage would leave the count one ahead for good
  if (e->n_prepared >= ffm_engine::kSets - 1) return fail(FFM_E_CAPACITY, "three prepared blocks are already waiting");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  SlotClaim claim;
  if ((rc = claim_slot(e, host, weight, zero_copy, &claim, resident))) return rc;
  const int this_slot = claim.slot;
  ffm_engine::Slot &sl = e->slots[this_slot];
  // its grouping, behind its own upload on the prep stream: planned here, submitted with the upload
  PrepPlan plan;
  if ((rc = prepare_plan(e, Rows{n_rows, nnz, sl.row_ptr, claim.has_field ? sl.field : nullptr, sl.feat, sl.val, nullptr}, &plan)))
    return rc;
  const int64_t seq = e->n_staged_total + 1;
  const int grid_pull = e->grid_pull;
  const bool timed = e->prof_on;  // (then submit runs the job on this thread)
  hipEvent_t free_ev = claim.was_used ? sl.free_ev : nullptr;
  // (val == NULL: the upload writes the slot's values -- every time, whatever the slot held before)
  float *const ones = sl.val;
  const unsigned n_ones = val ? 0u : static_cast<unsigned>(nnz);
  // FFM_FLAG_NORM_ROWS: the slot's values in place, right behind the upload that writes them and the ids
  const NormJob norm = e->norm_rows_on ? norm_job(e, Rows{n_rows, nnz, sl.row_ptr, claim.has_field ? sl.field : nullptr, sl.feat, sl.val, nullptr}, sl.val)
                                       : NormJob{};
  rc = e->submit([e, this_slot, free_ev, hjob = claim.job, rare = claim.rare, bucket = claim.bucket, plan, seq, grid_pull, timed, ones, n_ones, norm, ready]() -> int {
    ScopedTimer tm("stage:submit");
    ffm_engine::Slot &s2 = e->slots[this_slot];
    int rc2 = FFM_OK;
    auto body = [&]() -> int {
      HIP_TRY(hipSetDevice(e->cfg.device_id));
      if (free_ev) HIP_TRY(hipStreamWaitEvent(e->prep, free_ev, 0));  // nothing reads its device arrays
      if (ready) HIP_TRY(hipStreamWaitEvent(e->prep, ready, 0));  // (a resident block: its last take has run)
      // (long steps: the upload too waits for the running block's row kernel to end -- beside the update
      // launches it costs nothing, beside the row kernel, which is bound by the bytes it moves, it does)
      if (e->pull_after_row && plan.ws >= 0) HIP_TRY(hipStreamWaitEvent(e->prep, e->prep_after_row ? e->ev_row_done[plan.ws] : e->ev_set_free[plan.ws], 0));
      launch_upload(e, e->prep, grid_pull, hjob, rare, bucket, ones, n_ones);
      if (e->norm_rows_on) launch_normalize_rows(e, e->prep, norm);  // (on the slot's device copy: the caller's arrays are never written)
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
  slot_commit(e, claim, host, longest, weight != nullptr, zero_copy);
  e->staged[e->n_staged++] = this_slot;
  return FFM_OK;
}
int ffm_engine_stage_batch_weighted(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr,
                                    const int32_t *field, const int32_t *feat, const float *val,
                                    const int32_t *label, const float *weight, int32_t zero_copy) {
  SERVE_REFUSE(e, "training");  // (staging is training's: prediction stages through predict_batch_async)
  MASK_REFUSE(e, "training");
  int32_t nnz = 0;
  int longest = 1;
  int rc = validate_host_block(e, n_rows, row_ptr, &field, feat, val, &nnz, &longest, true);
  if (rc) return rc;
  if (n_rows > 0 && !label) return fail(FFM_E_INVALID, "training needs labels");
  if (n_rows == 0) weight = nullptr;
  if (weight) {  // refused here, on the caller's thread, before anything of the block is queued
    if ((rc = validate_host_weights(n_rows, weight))) return rc;
    if (zero_copy && !mapped16_or_refuse(weight, "a zero_copy weight array")) return FFM_E_INVALID;
  }
  return stage_block_from(e, Rows{n_rows, nnz, row_ptr, field, feat, val, label}, longest, weight, zero_copy);
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

// Phase 1 (grouping is done: refresh + forward) on the oldest staged block; opts.row_cap: set here, the slot's.
static int forward_staged(ffm_engine *e, float *partial_logit, ForwardOpts opts) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  SERVE_REFUSE(e, "training");
  MASK_REFUSE(e, "training");
  if (e->n_staged == 0) return fail(FFM_E_INVALID, "no staged block");
  if (e->has_pending) return fail(FFM_E_INVALID, "the previous block still awaits train_update");
  const int slot = e->staged[0];
  ffm_engine::Slot &sl = e->slots[slot];
  opts.row_cap = sl.row_cap;
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  if (int rc_w = e->wait_issued(sl.seq)) return rc_w;  // its upload + grouping launches are out
  // its grouping (behind the upload on the prep stream, or waiting for it there) implies the upload:
  // the main stream waits for ev_copied itself only when that grouping was discarded
  if (!(e->n_prepared > 0 && same_block(e->prepared_rows[0], slot_rows(sl, nullptr))))
    HIP_TRY(hipStreamWaitEvent(e->stream, sl.ev_copied, 0));
  int rc = train_forward_core(e, slot_rows(sl, sl.label), sl.has_weight ? sl.weight : nullptr, partial_logit, opts);
  if (rc) return rc;
  for (int i = 1; i < e->n_staged; i++) e->staged[i - 1] = e->staged[i];
  e->n_staged--;
  e->cur_slot = slot;  // released (ev_trained) by the train_update that follows
  return FFM_OK;
}
int ffm_engine_train_forward_staged(ffm_engine *e, float *partial_logit) {
  return forward_staged(e, partial_logit, ForwardOpts{});
}

// Whole step (ffm_engine_train_batch_device) on the oldest staged block.
int ffm_engine_train_staged(ffm_engine *e, float *logit_out, double *loss_sum_out) {
  if (e && e->m.n_shards > 1)
    return fail(FFM_E_INVALID, "sharded engines train with train_forward_staged + all-reduce + train_update");
  int rc = forward_staged(e, nullptr, ForwardOpts{0, true, logit_out});
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
    int rc = predict_core(e, slot_rows(sl, labelled ? sl.label : nullptr), output_prob, e->d_out,
                          labelled ? e->d_loss_sum : nullptr, sl.row_cap);
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
// (the entry point's steps behind the validation of `host`; resident / ready: as stage_block_from takes them)
static int predict_block_from(ffm_engine *e, const Rows &host, int longest, int32_t zero_copy, bool resident, hipEvent_t ready,
                              int32_t output_prob, float *scores_host) {
  const auto [n_rows, nnz, row_ptr, field, feat, val, label] = host;
  int rc;
  if (e->m.n_shards > 1) return fail(FFM_E_INVALID, "a sharded engine predicts through predict_batch_device + predict_finish_device");
  if (e->n_staged > 0 || e->has_pending) return fail(FFM_E_INVALID, "staged training blocks are still waiting");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  // (refused before the upload is launched: that kernel publishes the block's number)
  float *scores_dev = nullptr;
  if (scores_host && !(scores_dev = static_cast<float *>(mapped16_or_refuse(scores_host, "scores_host")))) return FFM_E_INVALID;
  if ((rc = e->drain())) return rc;
  SlotClaim claim;
  if ((rc = claim_slot(e, host, nullptr, zero_copy, &claim, resident))) return rc;
  const int this_slot = claim.slot;
  ffm_engine::Slot &sl = e->slots[this_slot];
  if (claim.was_used && sl.free_ev) HIP_TRY(hipStreamWaitEvent(e->prep, sl.free_ev, 0));  // nothing reads its device arrays
  if (ready) HIP_TRY(hipStreamWaitEvent(e->prep, ready, 0));  // (a resident block: its last take has run)
  // (no values came: the upload writes the slot's)
  launch_upload(e, e->prep, e->grid_pull, claim.job, claim.rare, claim.bucket, sl.val, val ? 0u : static_cast<unsigned>(nnz));
  if (e->norm_rows_on)  // (FFM_FLAG_NORM_ROWS: the slot's values in place, behind the upload)
    launch_normalize_rows(e, e->prep, norm_job(e, Rows{n_rows, nnz, sl.row_ptr, claim.has_field ? sl.field : nullptr, sl.feat, sl.val, nullptr}, sl.val));
  HIP_TRY(hipEventRecord(sl.ev_copied, e->prep));
  slot_commit(e, claim, host, longest, false, zero_copy);
  {
    std::lock_guard<std::mutex> lock(e->wmu);
    e->staged_issued = sl.seq;
  }
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
int ffm_engine_predict_batch_async_scores(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr,
                                          const int32_t *field, const int32_t *feat, const float *val,
                                          const int32_t *label, int32_t zero_copy, int32_t output_prob,
                                          float *scores_host) {
  int32_t nnz = 0;
  int longest = 1;
  // (hold_eval: the deferred block waits until this one's upload is submitted)
  int rc = validate_host_block(e, n_rows, row_ptr, &field, feat, val, &nnz, &longest, true, true);
  if (rc) return rc;
  return predict_block_from(e, Rows{n_rows, nnz, row_ptr, field, feat, val, label}, longest, zero_copy, false, nullptr, output_prob, scores_host);
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
