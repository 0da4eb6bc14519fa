// engine_metrics.h -- the AUC channels behind ffm_engine_metrics_* (include/ffm_engine.h "Metrics"):
// a score histogram per channel in HBM, filled by metric_hist_kernel (kernels_metric.h) on the
// engine's stream wherever a labelled logit is whole, reduced on the host in integers (metrics_host.h).
// Part of engine.hip's translation unit (included inside its extern "C" block).

// ---- metrics -------------------------------------------------------------------------------

static_assert(kMetricBins == FFM_METRIC_BINS, "the kernel and the ABI agree on the bins");
static constexpr size_t kMetricWords = 2 * static_cast<size_t>(kMetricBins) + 1;  // pos, neg, n_nan

// One launch per labelled block and channel, only when the channel is on (off: nothing happens).
static void launch_metric(ffm_engine *e, int channel, int n_rows, const float *score, int is_prob, const int *label) {
  const ffm_engine::MetricChannel &ch = e->metric[channel];
  if (!ch.on || n_rows <= 0 || !label) return;
  LAUNCH(e, K_METRIC, metric_hist_kernel, cdiv(n_rows, kMetricThreads), kMetricThreads, 0, n_rows, score, is_prob, label,
         ch.hist, ch.hist + kMetricBins, ch.hist + 2 * static_cast<size_t>(kMetricBins));
}

int ffm_engine_metrics_enable(ffm_engine *e, int32_t channel_mask) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  if (channel_mask < 0 || channel_mask > 3) return fail(FFM_E_INVALID, "channel_mask: bit 0 = eval, bit 1 = train");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  // a deferred evaluation block belongs to the setting it was handed over under
  if (int rc_e = eval_launch_pending(e)) return rc_e;
  for (int c = 0; c < 2; c++) {
    ffm_engine::MetricChannel &ch = e->metric[c];
    const bool want = (channel_mask >> c) & 1;
    if (want && !ch.on) {
      if (!ch.hist)
        if (int rc = e->alloc(&ch.hist, kMetricWords)) return rc;
      HIP_TRY(hipMemsetAsync(ch.hist, 0, kMetricWords * sizeof(unsigned long long), e->stream));
    }
    ch.on = want;
  }
  return FFM_OK;
}

// The channel's counters as the stream has them now, into host memory: [pos | neg | n_nan].  They are
// first copied aside on the device (the 64 MiB staging buffer of get / set), so that a reset can follow
// at once on the stream and blocks queued after this call never show in what is read.
static int metrics_snapshot(ffm_engine *e, int32_t channel, bool reset, std::vector<unsigned long long> *host) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  if (channel < 0 || channel > 1) return fail(FFM_E_INVALID, "channel: 0 = eval, 1 = train");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  if (int rc_e = eval_launch_pending(e)) return rc_e;
  ffm_engine::MetricChannel &ch = e->metric[channel];
  if (!ch.on) return fail(FFM_E_INVALID, "this metrics channel is off (ffm_engine_metrics_enable)");
  const size_t bytes = kMetricWords * sizeof(unsigned long long);
  if (bytes > static_cast<size_t>(e->stage_floats) * sizeof(float)) return fail(FFM_E_UNSUPPORTED, "staging buffer too small");
  try { host->assign(kMetricWords, 0ull); } catch (const std::bad_alloc &) { return fail(FFM_E_NOMEM, "host allocation failed"); }
  HIP_TRY(hipMemcpyAsync(e->d_stage, ch.hist, bytes, hipMemcpyDeviceToDevice, e->stream));
  if (reset) HIP_TRY(hipMemsetAsync(ch.hist, 0, bytes, e->stream));
  HIP_TRY(hipMemcpyAsync(host->data(), e->d_stage, bytes, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return FFM_OK;
}

int ffm_engine_metrics_from_histogram(const uint64_t *pos, const uint64_t *neg, int64_t n_bins,
                                      int64_t n_nan, ffm_metrics *out) {
  const int rc = ffm_metrics_host::from_histogram(pos, neg, n_bins, n_nan, out);
  return rc ? fail(rc, "null array, null output or negative count") : FFM_OK;
}

int ffm_engine_metrics_read(ffm_engine *e, int32_t channel, int32_t reset, ffm_metrics *out) {
  if (!out) return fail(FFM_E_INVALID, "null output");
  std::vector<unsigned long long> h;
  if (int rc = metrics_snapshot(e, channel, reset != 0, &h)) return rc;
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the counters are 64-bit");
  const uint64_t *w = reinterpret_cast<const uint64_t *>(h.data());
  return ffm_engine_metrics_from_histogram(w, w + kMetricBins, kMetricBins,
                                           static_cast<int64_t>(w[2 * static_cast<size_t>(kMetricBins)]), out);
}

int ffm_engine_metrics_histogram(ffm_engine *e, int32_t channel, uint64_t *pos, uint64_t *neg) {
  std::vector<unsigned long long> h;
  if (int rc = metrics_snapshot(e, channel, false, &h)) return rc;
  if (pos) std::memcpy(pos, h.data(), sizeof(uint64_t) * kMetricBins);
  if (neg) std::memcpy(neg, h.data() + kMetricBins, sizeof(uint64_t) * kMetricBins);
  return FFM_OK;
}
