// engine_hash.h -- FFM_FLAG_HASH_IDS: feature ids hashed into their field's id range on the device
// (csrc/hash_ids.h; include/ffm_engine.h "Hashed ids").  The in-place kernel of the synchronous path and
// of ffm_engine_hash_ids_device, and the host twin.  (The upload kernel's hashed variants: kernels_stage.h.)
// Part of engine.hip's translation unit (included inside its extern "C" block).

// feat_out[p] = hash(field[p], feat_in[p]) for p < nnz; in place (feat_out == feat_in) is fine: a lane
// reads its entries before it writes them and no lane reads another's.  A lane carries four entries as
// 16-byte vectors (vec != 0: every array is 16-byte aligned), what is left goes entry by entry.
// field == nullptr: FFM rows of one entry per field in field order; LR / FM have no fields.
__global__ __launch_bounds__(256) void hash_ids_kernel(ftrl_hash::Map hm, unsigned nnz, const int *field, const int *feat_in,
                                                       int *feat_out, int vec) {
  const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  const unsigned n4 = vec ? nnz >> 2 : 0u, F = static_cast<unsigned>(hm.n_fields);
  for (unsigned i = tid; i < n4; i += stride) {
    const int4 ft = reinterpret_cast<const int4 *>(feat_in)[i];
    const int4 fl = field ? reinterpret_cast<const int4 *>(field)[i] : hm.ffm ? ftrl_hash::hash_implicit_fields4(i, F) : make_int4(0, 0, 0, 0);
    reinterpret_cast<int4 *>(feat_out)[i] = ftrl_hash::hash_entries4(hm, fl, ft);
  }
  for (unsigned p = (n4 << 2) + tid; p < nnz; p += stride)
    feat_out[p] = ftrl_hash::hash_entry(hm, field ? field[p] : hm.ffm ? static_cast<int>(p % F) : 0, feat_in[p]);
}

// val: the block's values beside feat_in (the synchronous copies), mapped in place by an engine with a bucket table
// (ffm_engine_set_buckets: the bucketing kernel, kernels_valhist.h); nullptr: ids alone, as they always went.
// The whole mapping of an FFM engine with a bucket table: bucket, fold, hash; val moves with feat.
static void launch_bucket_ids(ffm_engine *e, hipStream_t st, int32_t nnz, const int32_t *field, const int32_t *feat_in, int32_t *feat_out,
                              const float *val_in, float *val_out) {
  if (nnz <= 0) return;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(field) | reinterpret_cast<uintptr_t>(feat_in) | reinterpret_cast<uintptr_t>(feat_out) |
                         reinterpret_cast<uintptr_t>(val_in) | reinterpret_cast<uintptr_t>(val_out);
  const int vec = (bits & 15u) == 0 ? 1 : 0;
  const int lanes = vec ? cdiv(nnz, 4) : nnz;
  hipLaunchKernelGGL(hash_ids_bucket_kernel, dim3(std::max(1, std::min(1024, cdiv(lanes, 256)))), dim3(256), 0, st, e->hm, e->rare, e->buckets,
                     static_cast<unsigned>(nnz), field, feat_in, feat_out, reinterpret_cast<const unsigned *>(val_in),
                     reinterpret_cast<unsigned *>(val_out), vec);
}

static void launch_hash_ids(ffm_engine *e, hipStream_t st, int32_t nnz, const int32_t *field, const int32_t *feat_in, int32_t *feat_out,
                            float *val = nullptr) {
  if (nnz <= 0) return;
  if (val && e->buckets.n_edges) {
    launch_bucket_ids(e, st, nnz, field, feat_in, feat_out, val, val);
    return;
  }
  const uintptr_t bits = reinterpret_cast<uintptr_t>(field) | reinterpret_cast<uintptr_t>(feat_in) | reinterpret_cast<uintptr_t>(feat_out);
  const int vec = (bits & 15u) == 0 ? 1 : 0;
  const int lanes = vec ? cdiv(nnz, 4) : nnz;
  if (e->rare.words)  // (ffm_engine_set_rare_fold: the folding kernel, kernels_idcount.h)
    hipLaunchKernelGGL(hash_ids_rare_kernel, dim3(std::max(1, std::min(1024, cdiv(lanes, 256)))), dim3(256), 0, st, e->hm, e->rare,
                       static_cast<unsigned>(nnz), field, feat_in, feat_out, vec);
  else
    hipLaunchKernelGGL(hash_ids_kernel, dim3(std::max(1, std::min(1024, cdiv(lanes, 256)))), dim3(256), 0, st, e->hm,
                       static_cast<unsigned>(nnz), field, feat_in, feat_out, vec);
}

// For callers of the _device entry points, which take ids as they are: the engine's mapping applied to a
// block that is already in HBM.  Asynchronous on the engine's stream, like those entry points.
int ffm_engine_hash_ids_device(ffm_engine *e, int32_t nnz, const int32_t *field, const int32_t *feat_in, int32_t *feat_out) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  if (nnz < 0) return fail(FFM_E_INVALID, "negative nnz");
  if (nnz > 0 && (!feat_in || !feat_out)) return fail(FFM_E_INVALID, "null id array");
  if (!e->hash_ids) return fail(FFM_E_INVALID, "this engine was created without FFM_FLAG_HASH_IDS");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  if (int rc_e = eval_launch_pending(e)) return rc_e;
  launch_hash_ids(e, e->stream, nnz, e->m.type == FFM_MODEL_FFM ? field : nullptr, feat_in, feat_out);
  HIP_TRY(hipGetLastError());
  return FFM_OK;
}

// What a flagged engine's ids are checked for: shapes, and no field of width 0 (nothing can land in it).
static int hash_ids_check(int32_t model_type, int32_t n_feats, int32_t n_fields, const int32_t *field_start) {
  if (model_type < FFM_MODEL_LR || model_type > FFM_MODEL_FFM) return fail(FFM_E_INVALID, "invalid model_type, expect LR(0), FM(1) or FFM(2)");
  if (n_feats <= 0) return fail(FFM_E_INVALID, "n_feats must be positive");
  if (model_type != FFM_MODEL_FFM) return FFM_OK;
  if (n_fields <= 0) return fail(FFM_E_INVALID, "n_fields must be positive for FFM");
  if (!field_start) return FFM_OK;
  bool ok = field_start[0] == 0 && field_start[n_fields] == n_feats;
  for (int f = 0; f < n_fields; f++) ok = ok && field_start[f] <= field_start[f + 1];
  if (!ok) return fail(FFM_E_INVALID, "field_start must ascend from 0 to n_feats");
  for (int f = 0; f < n_fields; f++)
    if (field_start[f] == field_start[f + 1])
      return fail(FFM_E_INVALID, "hashed ids need every field to own at least one id: field " + std::to_string(f) + " has width 0");
  return FFM_OK;
}

// The same mapping on the host (no device needed): the device's bits (csrc/hash_ids.h).
int ffm_engine_hash_ids_host(int32_t model_type, int32_t n_feats, int32_t n_fields, const int32_t *field_start, int32_t nnz,
                             const int32_t *field, const int32_t *feat_in, int32_t *feat_out) {
  if (int rc = hash_ids_check(model_type, n_feats, n_fields, field_start)) return rc;
  if (nnz < 0) return fail(FFM_E_INVALID, "negative nnz");
  if (nnz > 0 && (!feat_in || !feat_out)) return fail(FFM_E_INVALID, "null id array");
  const bool ffm = model_type == FFM_MODEL_FFM;
  const ftrl_hash::Map hm{ffm ? field_start : nullptr, n_feats, ffm ? n_fields : 1, ffm ? 1 : 0};
  for (int32_t p = 0; p < nnz; p++)
    feat_out[p] = ftrl_hash::hash_entry(hm, !ffm ? 0 : field ? field[p] : p % n_fields, feat_in[p]);
  return FFM_OK;
}
