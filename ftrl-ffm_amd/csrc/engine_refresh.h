// engine_refresh.h -- ffm_engine_refresh_weights: every stored weight from its accumulators, in one
// streaming pass over what the engine stores (kernels_refresh.h), and the six counts of what it saw.
// Part of engine.hip's translation unit (included inside its extern "C" block).

static_assert(sizeof(ffm_refresh_stats) == RC_COUNT * sizeof(int64_t), "the kernel and the ABI agree on the counters");

int ffm_engine_refresh_weights(ffm_engine *e, ffm_refresh_stats *out) {
  if (out) std::memset(out, 0, sizeof(*out));
  if (!e) return fail(FFM_E_INVALID, "null engine");
  SERVE_REFUSE(e, "ffm_engine_refresh_weights");
  if (e->has_pending) return fail(FFM_E_INVALID, "the previous block still awaits train_update");
  if (e->m.n_shards > 1 && e->n_staged > 0)
    return fail(FFM_E_INVALID, "a shard's staged blocks are trained by its group: ffm_group_refresh_weights, or flush first");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  // everything handed over so far is part of the model the pass sees, as for ffm_engine_changed_features:
  // the deferred evaluation block (scored with the weights as they were), the staged training blocks a
  // flush would train (their losses stay in the flush's sum), the staging thread, the device's flags
  if (int rc_e = eval_launch_pending(e)) return rc_e;
  while (e->n_staged > 0)
    if (int rc_t = train_one_staged(e)) return rc_t;
  if (int rc_d = check_device_errors(e)) return rc_d;
  if (!e->d_refresh)
    if (int rc = e->alloc(&e->d_refresh, static_cast<size_t>(RC_COUNT))) return rc;
  const auto kernel = e->m.row_len % 4 == 0 ? refresh_weights_kernel<true> : refresh_weights_kernel<false>;
  if (e->refresh_grid == 0) {
    // as many workgroups as the chip holds at once (every workgroup does the same number of turns, so a
    // second, partly filled round would only lengthen the pass)
    int cus = 0, per_cu = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->cfg.device_id));
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kRefreshThreads, 0));
    e->refresh_grid = std::max(1, cus) * std::max(1, per_cu);
  }
  // a persistent grid: never more workgroups than the chip holds, fewer only when the model has fewer lanes' work
  const int64_t lat_items = e->n_records * (e->m.row_len % 4 == 0 ? e->m.row_len / 4 : e->m.row_len);
  const int64_t items = std::max<int64_t>(lat_items, (static_cast<int64_t>(e->m.n_feats) + 4) / 4);
  const int grid = static_cast<int>(std::min<int64_t>(e->refresh_grid, std::max<int64_t>(1, (items + kRefreshThreads - 1) / kRefreshThreads)));
  HIP_TRY(hipMemsetAsync(e->d_refresh, 0, RC_COUNT * sizeof(unsigned long long), e->stream));
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kRefreshThreads), 0, e->stream, e->m, e->n_records, e->d_refresh);
  HIP_TRY(hipGetLastError());
  unsigned long long h[RC_COUNT] = {};
  HIP_TRY(hipMemcpyAsync(h, e->d_refresh, sizeof(h), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (out) {
    out->lin_live = static_cast<int64_t>(h[RC_LIN_LIVE]);
    out->lin_nonzero = static_cast<int64_t>(h[RC_LIN_NONZERO]);
    out->lin_moved = static_cast<int64_t>(h[RC_LIN_MOVED]);
    out->lat_live = static_cast<int64_t>(h[RC_LAT_LIVE]);
    out->lat_nonzero = static_cast<int64_t>(h[RC_LAT_NONZERO]);
    out->lat_moved = static_cast<int64_t>(h[RC_LAT_MOVED]);
  }
  return FFM_OK;
}
