// engine_mask.h -- pair masks on the prediction entry points (include/ffm_engine.h "Pair masks"): set checks what
// the masked kernel serves and what a mask must be, then copies the words to HBM behind everything queued so far;
// from then on launch_row_kernel (engine_step.h) runs ffm_row_mask_kernel (kernels_mask.h) for every predicted block,
// and whatever would run unmasked is refused (MASK_REFUSE, engine.hip).  An engine that never sets a mask allocates
// nothing and launches what it launched before.
// Part of engine.hip's translation unit (included inside its extern "C" block).

int ffm_engine_set_pair_mask(ffm_engine *e, const uint64_t *keep, int32_t n_fields) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  const ModelDev &m = e->m;
  if (!keep) {  // clears: blocks queued so far keep the mask they were queued under
    if (!e->pair_mask_on) return FFM_OK;
    HIP_TRY(hipSetDevice(e->cfg.device_id));
    if (int rc_e = eval_launch_pending(e)) return rc_e;
    e->pair_mask_on = false;
    return FFM_OK;
  }
  const std::string noun = "a pair mask";
  if (m.type != FFM_MODEL_FFM) return fail(FFM_E_UNSUPPORTED, noun + " is FFM only: LR and FM rows have no fields");
  if (m.n_shards > 1 || e->in_group)
    return fail(FFM_E_UNSUPPORTED, noun + " needs a whole model on one device (n_shards == 1, not a group's engine)");
  if (m.field_start || m.own_n || m.lin_own)
    return fail(FFM_E_UNSUPPORTED, noun + " needs full-length records (not a shard's compact storage)");
  if (m.n_fields > kMaskFields) return fail(FFM_E_UNSUPPORTED, noun + " supports at most 64 fields: a field's partners are one 64-bit word");
  if (!row_mask_fn(m.lat_fmt, m.n_factors))
    return fail(FFM_E_UNSUPPORTED, noun + " supports n_factors 4, 8, 16, 32 or 64 (the wave kernels' lane shapes)");
  if (!serving(e) && !e->predict_waves)
    return fail(FFM_E_UNSUPPORTED, noun + " needs the wave kernels, which FFM_PREDICT_WAVE=0 turned off when this engine was created");
  // ---- what a mask must be; a refused one leaves the previous mask in force
  if (n_fields != m.n_fields)
    return fail(FFM_E_INVALID, "the mask is for " + std::to_string(n_fields) + " fields, the engine has " + std::to_string(m.n_fields));
  for (int f = 0; f < n_fields; f++) {
    if (n_fields < 64 && (keep[f] >> n_fields) != 0)
      return fail(FFM_E_INVALID, "keep[" + std::to_string(f) + "] has a bit at or above n_fields");
    for (int g = 0; g < f; g++)
      if (((keep[f] >> g) & 1u) != ((keep[g] >> f) & 1u))
        return fail(FFM_E_INVALID, "the mask is not symmetric: bit " + std::to_string(g) + " of keep[" + std::to_string(f) +
                                       "] differs from bit " + std::to_string(f) + " of keep[" + std::to_string(g) + "]");
  }
  if (e->n_staged > 0 || e->has_pending) return fail(FFM_E_INVALID, "staged training blocks are still waiting");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  if (int rc_e = eval_launch_pending(e)) return rc_e;  // (a deferred block is scored under the mask it was queued under)
  if (!e->d_pair_mask)
    if (int rc = e->alloc(&e->d_pair_mask, static_cast<size_t>(kMaskFields))) return rc;
  PairMaskWords words{};
  std::copy(keep, keep + n_fields, words.w);
  // behind the kernels that still read the previous words, ahead of every block queued from now on
  hipLaunchKernelGGL(pair_mask_store_kernel, dim3(1), dim3(kMaskFields), 0, e->stream, words, e->d_pair_mask);
  HIP_TRY(hipGetLastError());
  std::copy(words.w, words.w + kMaskFields, e->pair_mask);
  e->pair_mask_on = true;
  return FFM_OK;
}

int ffm_engine_get_pair_mask(ffm_engine *e, uint64_t *keep_out, int32_t *is_set) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  if (is_set) *is_set = e->pair_mask_on ? 1 : 0;
  if (keep_out && e->m.n_fields <= kMaskFields)
    for (int f = 0; f < e->m.n_fields; f++) keep_out[f] = e->pair_mask_on ? e->pair_mask[f] : 0;
  return FFM_OK;
}
