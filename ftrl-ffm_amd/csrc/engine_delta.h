// engine_delta.h -- serving deltas (include/ffm_engine.h "Serving deltas"): ffm_engine_sync_weights brings a
// serving engine to a training engine's stored weights and keeps the set of features it had to move as a bitmap
// in HBM, ffm_engine_sync_moved lists that set, ffm_engine_get_rows_raw / set_rows_raw move rows in the table's
// own bits (kernels_delta.h).
// Part of engine.hip's translation unit (included inside its extern "C" block).

static_assert(sizeof(ffm_sync_stats) == SY_COUNT * sizeof(int64_t), "the kernel and the ABI agree on the counters");

int ffm_engine_sync_weights(ffm_engine *dst, ffm_engine *src, ffm_sync_stats *out) {
  if (out) std::memset(out, 0, sizeof(*out));
  if (!dst || !src) return fail(FFM_E_INVALID, "null engine");
  if (!serving(dst)) return fail(FFM_E_INVALID, "sync_weights: dst must be a serving engine (FFM_FLAG_SERVE_F32 / _F16)");
  if (serving(src)) return fail(FFM_E_INVALID, "sync_weights: src must be a training engine");
  if (src->m.type != FFM_MODEL_FFM || src->m.n_shards > 1)
    return fail(FFM_E_INVALID, "sync_weights: src must be a whole (unsharded) FFM model");
  if (src->m.n_feats != dst->m.n_feats || src->m.n_fields != dst->m.n_fields || src->m.n_factors != dst->m.n_factors)
    return fail(FFM_E_INVALID, "sync_weights: src and dst differ in (n_feats, n_fields, n_factors)");
  if (src->cfg.device_id != dst->cfg.device_id) return fail(FFM_E_INVALID, "sync_weights: src and dst live on different devices");
  if (src->has_pending) return fail(FFM_E_INVALID, "the previous block still awaits train_update");
  HIP_TRY(hipSetDevice(src->cfg.device_id));
  // the drains of ffm_engine_pack_weights: src as ffm_engine_refresh_weights drains it; dst's deferred
  // evaluation block sees dst as it was
  if (int rc_e = eval_launch_pending(src)) return rc_e;
  while (src->n_staged > 0)
    if (int rc_t = train_one_staged(src)) return rc_t;
  if (int rc_d = check_device_errors(src)) return rc_d;
  if (int rc_e = eval_launch_pending(dst)) return rc_e;
  const int64_t n_words = (static_cast<int64_t>(dst->m.n_feats) + 63) / 64;
  if (!dst->d_sync)
    if (int rc = dst->alloc(&dst->d_sync, static_cast<size_t>(SY_COUNT * kPackLine))) return rc;
  if (!dst->d_moved)
    if (int rc = dst->alloc(&dst->d_moved, static_cast<size_t>(n_words))) return rc;
  // src's stream is idle here (check_device_errors waits); the pass runs on dst's, behind what dst has queued.
  // A memory-bound stream: eight workgroups per CU at the most, the words beyond them walked grid-stride.
  int cus = 0;
  HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dst->cfg.device_id));
  const int grid = static_cast<int>(std::min<int64_t>(std::max(1, cus) * 8, std::max<int64_t>(1, (n_words + kSyncWaves - 1) / kSyncWaves)));
  HIP_TRY(hipMemsetAsync(dst->d_sync, 0, SY_COUNT * kPackLine * sizeof(unsigned long long), dst->stream));
  hipLaunchKernelGGL(serve_sync_fn(dst->m.lat_fmt), dim3(grid), dim3(kSyncThreads), 0, dst->stream, src->m, dst->m, n_words,
                     dst->d_moved, dst->d_sync);
  HIP_TRY(hipGetLastError());
  dst->synced = true;
  unsigned long long h[SY_COUNT * kPackLine] = {};
  HIP_TRY(hipMemcpyAsync(h, dst->d_sync, sizeof(h), hipMemcpyDeviceToHost, dst->stream));
  HIP_TRY(hipStreamSynchronize(dst->stream));
  if (out) {
    out->n_moved = static_cast<int64_t>(h[SY_MOVED * kPackLine]);
    out->n_lin_moved = static_cast<int64_t>(h[SY_LIN * kPackLine]);
    out->n_lat_moved = static_cast<int64_t>(h[SY_LAT * kPackLine]);
    out->bias_moved = static_cast<int64_t>(h[SY_BIAS * kPackLine]);
  }
  return FFM_OK;
}

int ffm_engine_sync_moved(ffm_engine *dst, int32_t *ids, int64_t cap, int64_t *n_moved) {
  if (n_moved) *n_moved = 0;
  if (!dst) return fail(FFM_E_INVALID, "null engine");
  if (!n_moved) return fail(FFM_E_INVALID, "null n_moved");
  if (ids && cap < 0) return fail(FFM_E_INVALID, "negative capacity");
  if (!serving(dst) || !dst->synced || !dst->d_moved)
    return fail(FFM_E_INVALID, "sync_moved: no ffm_engine_sync_weights has run on this engine");
  HIP_TRY(hipSetDevice(dst->cfg.device_id));
  const int64_t n_words = (static_cast<int64_t>(dst->m.n_feats) + 63) / 64;
  std::vector<unsigned long long> bits(static_cast<size_t>(n_words));
  HIP_TRY(hipMemcpyAsync(bits.data(), dst->d_moved, static_cast<size_t>(n_words) * sizeof(unsigned long long),
                         hipMemcpyDeviceToHost, dst->stream));
  HIP_TRY(hipStreamSynchronize(dst->stream));
  int64_t count = 0;
  for (unsigned long long b : bits) count += __builtin_popcountll(b);
  *n_moved = count;
  if (!ids) return FFM_OK;
  if (cap < count) return fail(FFM_E_CAPACITY, "ids holds " + std::to_string(cap) + " entries, " + std::to_string(count) + " features moved");
  int64_t at = 0;
  for (int64_t w = 0; w < n_words; w++)
    for (unsigned long long b = bits[static_cast<size_t>(w)]; b; b &= b - 1)
      ids[at++] = static_cast<int32_t>(w * 64 + __builtin_ctzll(b));
  return FFM_OK;
}

// ---- rows in the table's own bits ---------------------------------------------------------------------

static int rows_raw_transfer(ffm_engine *e, int32_t n, const int32_t *ids, float *lin_w, void *lat, bool to_host, const char *what) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  if (!serving(e))
    return fail(FFM_E_UNSUPPORTED, std::string(what) + " moves a serving engine's table in its own bits: a training engine "
                                       "has ffm_engine_get_rows / set_rows");
  if (n < 0 || (n > 0 && !ids)) return fail(FFM_E_INVALID, "bad feature id list");
  for (int32_t j = 0; j < n; j++)
    if (ids[j] < 0 || ids[j] >= e->m.n_feats) return fail(FFM_E_INVALID, "feature id out of range");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  if (int rc_e = eval_launch_pending(e)) return rc_e;  // (a deferred evaluation block sees the state as it was)
  const int64_t RL = e->logical_len;
  const size_t esize = e->m.lat_fmt == SERVE_F16 ? 2 : 4;
  // (the staging buffer holds stage_floats elements of 4 bytes: room for as many of 2)
  const int64_t per = std::min<int64_t>(ffm_engine::kIdsCap, RL > 0 ? e->stage_floats / RL : ffm_engine::kIdsCap);
  for (int64_t j0 = 0; j0 < n; j0 += per) {
    const int nf = static_cast<int>(std::min<int64_t>(per, n - j0));
    HIP_TRY(hipMemcpyAsync(e->d_ids, ids + j0, sizeof(int) * nf, hipMemcpyHostToDevice, e->stream));
    if (lin_w) {
      if (!to_host) HIP_TRY(hipMemcpyAsync(e->d_stage, lin_w + j0, sizeof(float) * nf, hipMemcpyHostToDevice, e->stream));
      hipLaunchKernelGGL(lin_rows_copy_kernel, dim3(cdiv(nf, 256)), dim3(256), 0, e->stream, e->m.lin_w, e->m.n_feats,
                         e->d_stage, e->d_ids, nf, to_host ? 1 : 0);
      if (to_host) HIP_TRY(hipMemcpyAsync(lin_w + j0, e->d_stage, sizeof(float) * nf, hipMemcpyDeviceToHost, e->stream));
      HIP_TRY(hipStreamSynchronize(e->stream));
    }
    if (lat && RL > 0) {
      char *const host = static_cast<char *>(lat) + static_cast<size_t>(j0) * RL * esize;
      const size_t bytes = static_cast<size_t>(nf) * RL * esize;
      if (!to_host) HIP_TRY(hipMemcpyAsync(e->d_stage, host, bytes, hipMemcpyHostToDevice, e->stream));
      hipLaunchKernelGGL(serve_rows_raw_fn(e->m.lat_fmt), dim3(1024), dim3(256), 0, e->stream, e->m,
                         static_cast<void *>(e->d_stage), e->d_ids, static_cast<int64_t>(nf), to_host ? 1 : 0);
      if (to_host) HIP_TRY(hipMemcpyAsync(host, e->d_stage, bytes, hipMemcpyDeviceToHost, e->stream));
      HIP_TRY(hipStreamSynchronize(e->stream));
    }
  }
  HIP_TRY(hipGetLastError());
  return FFM_OK;
}

int ffm_engine_get_rows_raw(ffm_engine *e, int32_t n, const int32_t *ids, float *lin_w, void *lat) {
  return rows_raw_transfer(e, n, ids, lin_w, lat, true, "ffm_engine_get_rows_raw");
}

int ffm_engine_set_rows_raw(ffm_engine *e, int32_t n, const int32_t *ids, const float *lin_w, const void *lat) {
  return rows_raw_transfer(e, n, ids, const_cast<float *>(lin_w), const_cast<void *>(lat), false, "ffm_engine_set_rows_raw");
}
