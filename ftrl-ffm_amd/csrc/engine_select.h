// engine_select.h -- which instantiation of a kernel family runs for a shape.  One host function per family maps
// the run-time facts to a typed kernel pointer, or to null for a combination that nothing launches (and that is
// therefore not in the code object).  The launches (engine_step.h, engine_serve.h) and the dynamic-LDS opt-in
// of ffm_engine_create (engine.hip: opt_in_lds) both ask here, so they cannot disagree about what exists.
// Part of engine.hip's translation unit (included inside its anonymous namespace).

// ---- the row kernels (kernels_row.h, kernels_fm.h) --------------------------------------------------------
// W...: nothing, or `const float *` -- the per-row sample weights of the instantiations that take them.
template <typename... W>
using FfmRowFn = void (*)(ModelDev, Rows, Scratch, int, float *, int, int, int, int, int, W...);
using FmRowFn = void (*)(ModelDev, Rows, Scratch, int, float *, int);
template <typename... W>
using FmRowWaveFn = void (*)(ModelDev, Rows, Scratch, int, float *, int, int, W...);
using FfmRefreshFn = void (*)(ModelDev, Scratch, int);

// whole: the template's WHOLE.  For k % 4 == 0 that is "this launch has the whole logit" (one shard's
// train_batch_device); the general-k training kernel is always the WHOLE one and takes own_tg as an argument.
// hold: 0, 2, 4, 6 or 8 held (n, z) vectors per thread (the in-row update's kernel only).
template <typename... W>
FfmRowFn<W...> ffm_row_fn(bool train, bool vec4, bool whole, int hold) {
  if (train && vec4 && whole) switch (hold) {
      case 0: return ffm_row_kernel<true, true, true, 0, W...>;
      case 2: return ffm_row_kernel<true, true, true, 2, W...>;
      case 4: return ffm_row_kernel<true, true, true, 4, W...>;
      case 6: return ffm_row_kernel<true, true, true, 6, W...>;
      case 8: return ffm_row_kernel<true, true, true, 8, W...>;
      default: return nullptr;
    }
  if (hold != 0) return nullptr;
  if (train && !vec4 && whole) return ffm_row_kernel<true, false, true, 0, W...>;
  if constexpr (sizeof...(W) == 0) {  // (weights go to the kernels that produce tmp_grad: none below does)
    if (train && vec4 && !whole) return ffm_row_kernel<true, true, false>;  // a shard's
    if (!train && !whole) return vec4 ? ffm_row_kernel<false, true> : ffm_row_kernel<false, false>;
  }
  return nullptr;
}
inline FmRowFn fm_row_fn(bool train) { return train ? fm_row_kernel<true> : fm_row_kernel<false>; }
template <typename... W>
FmRowWaveFn<W...> fm_row_wave_fn(bool train) {
  if (train) return fm_row_wave_kernel<true, W...>;
  if constexpr (sizeof...(W) == 0) return fm_row_wave_kernel<false>;
  return nullptr;
}
inline FfmRefreshFn ffm_refresh_fn(bool vec4) { return vec4 ? ffm_refresh_kernel<true> : ffm_refresh_kernel<false>; }

// ---- the FFM update (kernels_tile.h, kernels_update.h) ----------------------------------------------------
using UpdateAllFn = void (*)(ModelDev, Rows, Scratch, int, int, int, int, int, int, int, double *, double *, int);
using UpdateRowsFn = void (*)(ModelDev, Rows, Scratch);  // ffm_update_single_kernel, ffm_update_super_b_kernel

template <int NF>
UpdateAllFn update_all_kinds(int kinds) {
  switch (kinds) {
    case UPD_ALL: return ffm_update_all_kernel<NF>;
    case UPD_ALL & ~UPD_FEW: return ffm_update_all_kernel<NF, UPD_ALL & ~UPD_FEW>;  // a shard: few-occurrence features apart
    case UPD_HOT | UPD_SIDE: return ffm_update_all_kernel<NF, UPD_HOT | UPD_SIDE>;  // split: the main stream's
    case UPD_FEW | UPD_REST: return ffm_update_all_kernel<NF, UPD_FEW | UPD_REST>;  // side by side: aux3's
    case UPD_GIANT: return ffm_update_all_kernel<NF, UPD_GIANT>;
    case UPD_FEW: return ffm_update_all_kernel<NF, UPD_FEW>;    // one after another
    case UPD_REST: return ffm_update_all_kernel<NF, UPD_REST>;  // one after another
    default: return nullptr;
  }
}
// nf: tile_nf (1: k >= 16, 2: k = 8 / 12, 4: k = 4); kinds: the UPD_* ranges of the launch; waves: per workgroup.
inline UpdateAllFn update_all_fn(int nf, int kinds, int waves) {
  if (nf == 1 && kinds == UPD_ALL && waves == kWideWaves) return ffm_update_all_kernel<1, UPD_ALL, kWideWaves>;
  if (waves != tile_waves(nf)) return nullptr;
  return nf == 1 ? update_all_kinds<1>(kinds) : nf == 2 ? update_all_kinds<2>(kinds) : nf == 4 ? update_all_kinds<4>(kinds) : nullptr;
}
// span4: 16-byte vectors of a stored record -- a lane of the once-only kernel makes one trip per 64 of them
inline UpdateRowsFn update_single_fn(int span4) {
  return span4 <= 64 ? ffm_update_single_kernel<1> : span4 <= 128 ? ffm_update_single_kernel<2> : ffm_update_single_kernel<3>;
}
inline UpdateRowsFn update_super_b_fn(int nf) {
  return nf == 1 ? ffm_update_super_b_kernel<1> : nf == 2 ? ffm_update_super_b_kernel<2> : nf == 4 ? ffm_update_super_b_kernel<4> : nullptr;
}

// ---- the wave kernels: a row (a context, a candidate) per wave (kernels_wave.h, kernels_serve.h, kernels_ablate.h)
// The lane shape of n_factors, X(k, LPP, VPL, U): lanes per pair, vectors per lane, steps of loads in flight
// together.  These are the n_factors the wave kernels exist for; every selector below is null for any other.
#ifndef FFM_PRED_LPP
#define FFM_PRED_LPP 4  // k = 16: lanes per pair (1, 2, 4) ...
#endif
#ifndef FFM_PRED_U
#define FFM_PRED_U 4    // ... and steps of loads in flight together
#endif
#define FFM_LANE_SHAPES(X) \
  X(4, 1, 1, 4) X(8, 2, 1, 4) X(16, FFM_PRED_LPP, 4 / FFM_PRED_LPP, FFM_PRED_U) X(32, 8, 1, 2) X(64, 16, 1, 1)

using RowWaveFn = void (*)(ModelDev, Rows, Scratch, int, int, float *, int);  // ffm_row_wave_kernel: predict and serve alike
using ServeContextFn = void (*)(ModelDev, int, const int *, const int *, const int *, const float *, const int *, int,
                                CandCtx, int, int, int *);
using ServeCandidateFn = void (*)(ModelDev, int, const int *, CandCtx, Rows, int, int, int *, float *, int);

// fmt: ModelDev::lat_fmt -- SERVE_NONE (a training engine's records), SERVE_F32 or SERVE_F16 (a packed table of w).
// FFM_BY_FMT: a family of the packed tables alone (a context and a candidate exist on a serving engine only: null
// for SERVE_NONE); FFM_BY_ANY_FMT: one of all three (rows, field ablation).
#define FFM_BY_FMT(KERNEL, LPP, VPL, U) \
  (fmt == SERVE_F16 ? KERNEL<SERVE_F16, LPP, VPL, U> : fmt == SERVE_F32 ? KERNEL<SERVE_F32, LPP, VPL, U> : nullptr)
#define FFM_BY_ANY_FMT(KERNEL, LPP, VPL, U) \
  (fmt == SERVE_NONE ? KERNEL<SERVE_NONE, LPP, VPL, U> : FFM_BY_FMT(KERNEL, LPP, VPL, U))
inline RowWaveFn row_wave_fn(int fmt, int n_factors) {
  switch (n_factors) {
#define X(K, LPP, VPL, U) case K: return FFM_BY_ANY_FMT(ffm_row_wave_kernel, LPP, VPL, U);
    FFM_LANE_SHAPES(X)
#undef X
    default: return nullptr;
  }
}
// prediction under a pair mask (kernels_mask.h): ffm_row_wave_kernel's arguments, then the mask words in HBM
using RowMaskFn = void (*)(ModelDev, Rows, Scratch, int, int, float *, int, const unsigned long long *);
inline RowMaskFn row_mask_fn(int fmt, int n_factors) {
  switch (n_factors) {
#define X(K, LPP, VPL, U) case K: return FFM_BY_ANY_FMT(ffm_row_mask_kernel, LPP, VPL, U);
    FFM_LANE_SHAPES(X)
#undef X
    default: return nullptr;
  }
}
inline ServeContextFn serve_context_fn(int fmt, int n_factors) {
  switch (n_factors) {
#define X(K, LPP, VPL, U) case K: return FFM_BY_FMT(serve_context_kernel, LPP, VPL, U);
    FFM_LANE_SHAPES(X)
#undef X
    default: return nullptr;
  }
}
inline ServeCandidateFn serve_candidate_fn(int fmt, int n_factors) {
  switch (n_factors) {
#define X(K, LPP, VPL, U) case K: return FFM_BY_FMT(serve_candidate_kernel, LPP, VPL, U);
    FFM_LANE_SHAPES(X)
#undef X
    default: return nullptr;
  }
}
// field ablation (kernels_ablate.h)
using AblateWaveFn = void (*)(ModelDev, Rows, int *, int, int, float *, double *, int, int);
inline AblateWaveFn ablate_wave_fn(int fmt, int n_factors) {
  switch (n_factors) {
#define X(K, LPP, VPL, U) case K: return FFM_BY_ANY_FMT(ffm_ablate_wave_kernel, LPP, VPL, U);
    FFM_LANE_SHAPES(X)
#undef X
    default: return nullptr;
  }
}
// pair ablation (kernels_ablate_pairs.h): a lane keeps ceil(V / 64) running values in registers, V = F (F + 1) / 2,
// and their number is a template bound -- 2 (up to 15 fields), 13 (up to 40: the headline shape's 39 need all 13)
// or 33 (up to 64 fields).  A smaller model pays for the idle accumulators of its bound, never for scratch.
inline int ablate_pairs_rounds(int n_fields) {
  if (n_fields < 1 || n_fields > kPairFields) return 0;
  const int rounds = (pair_variants(n_fields) + 63) / 64;
  return rounds <= 2 ? 2 : rounds <= 13 ? 13 : 33;
}
template <int FMT, int LPP, int VPL, int U>
constexpr AblateWaveFn ablate_pairs_2 = ffm_ablate_pairs_kernel<FMT, LPP, VPL, U, 2>;
template <int FMT, int LPP, int VPL, int U>
constexpr AblateWaveFn ablate_pairs_13 = ffm_ablate_pairs_kernel<FMT, LPP, VPL, U, 13>;
template <int FMT, int LPP, int VPL, int U>
constexpr AblateWaveFn ablate_pairs_33 = ffm_ablate_pairs_kernel<FMT, LPP, VPL, U, 33>;
// rounds: ablate_pairs_rounds(n_fields); the arguments are ffm_ablate_wave_kernel's
inline AblateWaveFn ablate_pairs_fn(int fmt, int n_factors, int rounds) {
  switch (n_factors) {
#define X(K, LPP, VPL, U)                                                            \
  case K:                                                                            \
    return rounds == 2    ? FFM_BY_ANY_FMT(ablate_pairs_2, LPP, VPL, U)              \
           : rounds == 13 ? FFM_BY_ANY_FMT(ablate_pairs_13, LPP, VPL, U)             \
           : rounds == 33 ? FFM_BY_ANY_FMT(ablate_pairs_33, LPP, VPL, U) : nullptr;
    FFM_LANE_SHAPES(X)
#undef X
    default: return nullptr;
  }
}
// the pruning curve (kernels_curve.h): ffm_ablate_wave_kernel's arguments, then the level table and the cuts in HBM
using CurveWaveFn = void (*)(ModelDev, Rows, int *, int, int, float *, double *, int, int, CurveDev);
inline CurveWaveFn curve_wave_fn(int fmt, int n_factors) {
  switch (n_factors) {
#define X(K, LPP, VPL, U) case K: return FFM_BY_ANY_FMT(ffm_curve_wave_kernel, LPP, VPL, U);
    FFM_LANE_SHAPES(X)
#undef X
    default: return nullptr;
  }
}
#undef FFM_BY_ANY_FMT
#undef FFM_BY_FMT
#undef FFM_LANE_SHAPES

// ---- serving deltas (kernels_delta.h): one instantiation per format of the packed table ---------------------
using ServeSyncFn = void (*)(ModelDev, ModelDev, int64_t, unsigned long long *, unsigned long long *);
using ServeRowsRawFn = void (*)(ModelDev, void *, const int *, int64_t, int);
inline ServeSyncFn serve_sync_fn(int fmt) {
  return fmt == SERVE_F16 ? serve_sync_kernel<SERVE_F16> : fmt == SERVE_F32 ? serve_sync_kernel<SERVE_F32> : nullptr;
}
inline ServeRowsRawFn serve_rows_raw_fn(int fmt) {  // elements of 2 or 4 bytes, moved as they are
  return fmt == SERVE_F16 ? serve_rows_raw_kernel<unsigned short> : fmt == SERVE_F32 ? serve_rows_raw_kernel<unsigned> : nullptr;
}
