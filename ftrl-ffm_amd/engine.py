"""ctypes binding of the C ABI in include/ffm_engine.h (libffm_engine.so, hand-written HIP for
gfx950).  This is plumbing only: every call goes straight to the shared library, and there is no
CPU fallback -- if the library or a GPU is missing, loading / Engine() raises.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libffm_engine.so")

LR, FM, FFM = 0, 1, 2
MODEL_TYPES = {"LR": LR, "FM": FM, "FFM": FFM}
FLAG_SKIP_INIT = 1
FLAG_LEARN = 4
FLAG_HASH_IDS = 8
FLAG_SERVE_F32, FLAG_SERVE_F16 = 16, 32
FLAG_NORM_ROWS = 64
SERVE_FLAGS = {None: 0, "none": 0, "f32": FLAG_SERVE_F32, "f16": FLAG_SERVE_F16}
E_INVALID, E_DEVICE, E_NOMEM, E_CAPACITY, E_UNSUPPORTED = -1, -2, -3, -4, -5  # FFM_E_*

_i32p = ctypes.POINTER(ctypes.c_int32)
_f32p = ctypes.POINTER(ctypes.c_float)
_f64p = ctypes.POINTER(ctypes.c_double)
_vp = ctypes.c_void_p


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("ffm_engine error %d: %s" % (code, msg))
        self.code = code


class Config(ctypes.Structure):
    """struct ffm_engine_config (include/ffm_engine.h)."""
    _fields_ = [("model_type", ctypes.c_int32), ("n_feats", ctypes.c_int32),
                ("n_fields", ctypes.c_int32), ("n_factors", ctypes.c_int32),
                ("w_alpha", ctypes.c_float), ("w_beta", ctypes.c_float),
                ("w_l1", ctypes.c_float), ("w_l2", ctypes.c_float),
                ("init_mean", ctypes.c_float), ("init_stddev", ctypes.c_float),
                ("seed", ctypes.c_uint64), ("max_batch_rows", ctypes.c_int32),
                ("max_batch_nnz", ctypes.c_int32), ("device_id", ctypes.c_int32),
                ("n_shards", ctypes.c_int32), ("shard_rank", ctypes.c_int32),
                ("stream", ctypes.c_void_p), ("flags", ctypes.c_int32),
                ("max_row_nnz", ctypes.c_int32), ("field_start", _i32p),
                ("reserved", ctypes.c_int32 * 4)]


class Metrics(ctypes.Structure):
    """struct ffm_metrics (include/ffm_engine.h "Metrics")."""
    _fields_ = [("n_pos", ctypes.c_int64), ("n_neg", ctypes.c_int64), ("n_nan", ctypes.c_int64),
                ("n_mixed_bins", ctypes.c_int64), ("auc", ctypes.c_double), ("auc_slack", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class KeyedMetrics(ctypes.Structure):
    """struct ffm_keyed_metrics (include/ffm_engine.h "Metrics", keyed capture)."""
    _fields_ = [(k, ctypes.c_int64) for k in ("n_rows", "n_keys", "n_keys_mixed", "n_rows_mixed", "n_nan", "n_unkeyed",
                                              "n_overflow")] + [("gauc", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class RefreshStats(ctypes.Structure):
    """struct ffm_refresh_stats (include/ffm_engine.h "Refresh")."""
    _fields_ = [(k, ctypes.c_int64) for k in ("lin_live", "lin_nonzero", "lin_moved",
                                              "lat_live", "lat_nonzero", "lat_moved")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class PackStats(ctypes.Structure):
    """struct ffm_pack_stats (include/ffm_engine.h "Serving engines")."""
    _fields_ = [(k, ctypes.c_int64) for k in ("n_latent", "n_inexact", "n_to_inf", "n_to_zero")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class SyncStats(ctypes.Structure):
    """struct ffm_sync_stats (include/ffm_engine.h "Serving deltas")."""
    _fields_ = [(k, ctypes.c_int64) for k in ("n_moved", "n_lin_moved", "n_lat_moved", "bias_moved")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class TextBlock(ctypes.Structure):
    """struct ffm_text_block (include/ffm_engine.h "Text blocks")."""
    _fields_ = ([(k, ctypes.c_int64) for k in ("n_lines", "n_rows", "nnz", "n_slow", "first_slow_byte")] +
                [("overflow", ctypes.c_int32)] +
                [(k, ctypes.c_void_p) for k in ("row_ptr", "field", "feat", "label", "val")])

    def as_dict(self):
        return {k: (getattr(self, k) if t is ctypes.c_void_p else int(getattr(self, k))) for k, t in self._fields_}


class RowsBlock(ctypes.Structure):
    """struct ffm_rows_block (include/ffm_engine.h "Resident rows"): a block of rows in HBM."""
    _fields_ = ([(k, ctypes.c_int32) for k in ("n_rows", "nnz", "longest_row", "index")] + [("seq", ctypes.c_int64)] +
                [(k, ctypes.c_void_p) for k in ("row_ptr", "field", "feat", "label", "val", "ready")])


RAW_DTYPES = {"f32": np.float32, "f16": np.uint16}  # a serving table's own elements, per format

METRIC_EVAL, METRIC_TRAIN = 0, 1  # FFM_METRIC_*
METRIC_BINS = 1 << 20             # FFM_METRIC_BINS
_METRIC_CHANNELS = {"eval": METRIC_EVAL, "train": METRIC_TRAIN}
_u64p = ctypes.POINTER(ctypes.c_uint64)
_i64p = ctypes.POINTER(ctypes.c_int64)

# every symbol include/ffm_engine.h declares: (name, restype, argtypes)
_CSR = [_i32p, _i32p, _i32p, _f32p, _i32p]
_DCSR = [_vp, _vp, _vp, _vp, _vp]
ABI = [
    ("ffm_engine_default_config", None, [ctypes.POINTER(Config)]),
    ("ffm_engine_create", ctypes.c_int, [ctypes.POINTER(Config), ctypes.POINTER(_vp)]),
    ("ffm_engine_init_weights_host", ctypes.c_int,
     [ctypes.c_uint64, ctypes.c_float, ctypes.c_float, ctypes.c_int32, ctypes.c_int64,
      ctypes.c_int64, _f32p]),
    ("ffm_engine_destroy", None, [_vp]),
    ("ffm_engine_last_error", ctypes.c_char_p, []),
    ("ffm_engine_abi_version", ctypes.c_int, []),
    ("ffm_engine_block_segment", ctypes.c_int, []),
    ("ffm_engine_row_len", ctypes.c_int64, [_vp]),
    ("ffm_engine_default_batch_ramp", ctypes.c_int32, [ctypes.c_float]),
    ("ffm_engine_shard_plan", ctypes.c_int,
     [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _i32p, _i32p, _i32p]),
    ("ffm_engine_set_weights", ctypes.c_int, [_vp, _f32p, _f32p, _f32p]),
    ("ffm_engine_get_weights", ctypes.c_int, [_vp, _f32p, _f32p, _f32p]),
    ("ffm_engine_set_state", ctypes.c_int, [_vp] + [_f32p] * 6),
    ("ffm_engine_get_state", ctypes.c_int, [_vp] + [_f32p] * 6),
    ("ffm_engine_get_rows", ctypes.c_int, [_vp, ctypes.c_int32, _i32p] + [_f32p] * 6),
    ("ffm_engine_set_rows", ctypes.c_int, [_vp, ctypes.c_int32, _i32p] + [_f32p] * 6),
    ("ffm_engine_changed_features", ctypes.c_int,
     [_vp, _i32p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    ("ffm_engine_train_batch", ctypes.c_int, [_vp, ctypes.c_int32] + _CSR + [_f32p, _f64p]),
    ("ffm_engine_predict_batch", ctypes.c_int,
     [_vp, ctypes.c_int32] + _CSR + [ctypes.c_int32, _f32p, _f64p]),
    ("ffm_engine_train_batch_device", ctypes.c_int,
     [_vp, ctypes.c_int32, ctypes.c_int32] + _DCSR + [_vp, _vp]),
    ("ffm_engine_predict_batch_device", ctypes.c_int,
     [_vp, ctypes.c_int32, ctypes.c_int32] + _DCSR + [ctypes.c_int32, _vp, _vp]),
    ("ffm_engine_predict_finish_device", ctypes.c_int,
     [_vp, ctypes.c_int32, _vp, _vp, ctypes.c_int32, _vp, _vp]),
    ("ffm_engine_train_batch_async", ctypes.c_int, [_vp, ctypes.c_int32] + _CSR),
    ("ffm_engine_train_batch_async_pinned", ctypes.c_int, [_vp, ctypes.c_int32] + _CSR),
    ("ffm_engine_train_flush", ctypes.c_int, [_vp, _f64p]),
    ("ffm_engine_predict_batch_async", ctypes.c_int, [_vp, ctypes.c_int32] + _CSR + [ctypes.c_int32]),
    ("ffm_engine_predict_batch_async_scores", ctypes.c_int,
     [_vp, ctypes.c_int32] + _CSR + [ctypes.c_int32, ctypes.c_int32, _vp]),
    ("ffm_engine_blocks_scored", ctypes.c_int64, [_vp]),
    ("ffm_engine_stage_batch", ctypes.c_int, [_vp, ctypes.c_int32] + _CSR + [ctypes.c_int32]),
    ("ffm_engine_blocks_pulled", ctypes.c_int64, [_vp]),
    ("ffm_engine_train_forward_staged", ctypes.c_int, [_vp, _vp]),
    ("ffm_engine_train_staged", ctypes.c_int, [_vp, _vp, _vp]),
    ("ffm_engine_pin_host", ctypes.c_int, [_vp, ctypes.c_size_t]),
    ("ffm_engine_unpin_host", ctypes.c_int, [_vp]),
    ("ffm_engine_prepare_device", ctypes.c_int,
     [_vp, ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp, _vp]),
    ("ffm_engine_train_forward_device", ctypes.c_int,
     [_vp, ctypes.c_int32, ctypes.c_int32] + _DCSR + [_vp]),
    ("ffm_engine_train_update_device", ctypes.c_int, [_vp, _vp, _vp, _vp]),
    ("ffm_engine_fill_state", ctypes.c_int,
     [_vp, ctypes.c_uint64, ctypes.c_float, ctypes.c_float, ctypes.c_float]),
    ("ffm_engine_eval_sigmoid", ctypes.c_int, [_vp, ctypes.c_int32, _f32p, _f32p]),
    ("ffm_engine_sync", ctypes.c_int, [_vp]),
    ("ffm_engine_check_errors", ctypes.c_int, [_vp]),
    ("ffm_engine_stream", ctypes.c_void_p, [_vp]),
    ("ffm_engine_profile_enable", ctypes.c_int, [_vp, ctypes.c_int32]),
    ("ffm_engine_profile_read", ctypes.c_int,
     [_vp, _i32p, _f64p, ctypes.c_char_p, ctypes.c_size_t]),
    ("ffm_engine_profile_focus", ctypes.c_int, [_vp]),
    ("ffm_engine_profile_dump", ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_size_t]),
    ("ffm_engine_metrics_enable", ctypes.c_int, [_vp, ctypes.c_int32]),
    ("ffm_engine_metrics_read", ctypes.c_int,
     [_vp, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(Metrics)]),
    ("ffm_engine_metrics_histogram", ctypes.c_int, [_vp, ctypes.c_int32, _u64p, _u64p]),
    ("ffm_engine_metrics_from_histogram", ctypes.c_int,
     [_u64p, _u64p, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(Metrics)]),
    # the grouped AUC (include/ffm_engine.h "Metrics", keyed capture)
    ("ffm_engine_metrics_key_field", ctypes.c_int, [_vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64]),
    ("ffm_engine_metrics_read_keyed", ctypes.c_int, [_vp, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(KeyedMetrics)]),
    ("ffm_engine_metrics_keyed_table", ctypes.c_int,
     [_vp, ctypes.c_int32, ctypes.c_int64, _i32p, _i64p, _i64p, _u64p, _i64p]),
    ("ffm_engine_metrics_from_keyed", ctypes.c_int, [_i64p, _i64p, _u64p, ctypes.c_int64, ctypes.POINTER(KeyedMetrics)]),
    # several GPUs in one process (ffm_group_*)
    ("ffm_group_create", ctypes.c_int, [ctypes.POINTER(Config), ctypes.c_int32, _i32p, ctypes.POINTER(_vp)]),
    ("ffm_group_destroy", None, [_vp]),
    ("ffm_group_size", ctypes.c_int32, [_vp]),
    ("ffm_group_engine", ctypes.c_void_p, [_vp, ctypes.c_int32]),
    ("ffm_group_collective", ctypes.c_char_p, [_vp]),
    ("ffm_group_train_batch", ctypes.c_int, [_vp, ctypes.c_int32] + _CSR + [_f32p, _f64p]),
    ("ffm_group_train_batch_async", ctypes.c_int, [_vp, ctypes.c_int32] + _CSR + [ctypes.c_int32]),
    ("ffm_group_train_flush", ctypes.c_int, [_vp, _f64p]),
    ("ffm_group_blocks_pulled", ctypes.c_int64, [_vp]),
    ("ffm_group_predict_batch", ctypes.c_int,
     [_vp, ctypes.c_int32] + _CSR + [ctypes.c_int32, _f32p, _f64p]),
    ("ffm_group_metrics_enable", ctypes.c_int, [_vp, ctypes.c_int32]),
    ("ffm_group_metrics_read", ctypes.c_int,
     [_vp, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(Metrics)]),
    # sample weights: one float32 per row, after `label` (include/ffm_engine.h "Sample weights")
    ("ffm_engine_train_batch_weighted", ctypes.c_int, [_vp, ctypes.c_int32] + _CSR + [_f32p, _f32p, _f64p]),
    ("ffm_engine_train_batch_device_weighted", ctypes.c_int,
     [_vp, ctypes.c_int32, ctypes.c_int32] + _DCSR + [_vp, _vp, _vp]),
    ("ffm_engine_train_forward_device_weighted", ctypes.c_int,
     [_vp, ctypes.c_int32, ctypes.c_int32] + _DCSR + [_vp, _vp]),
    ("ffm_engine_stage_batch_weighted", ctypes.c_int, [_vp, ctypes.c_int32] + _CSR + [_vp, ctypes.c_int32]),
    ("ffm_engine_train_batch_async_weighted", ctypes.c_int,
     [_vp, ctypes.c_int32] + _CSR + [_vp, ctypes.c_int32]),
    ("ffm_group_train_batch_weighted", ctypes.c_int, [_vp, ctypes.c_int32] + _CSR + [_f32p, _f32p, _f64p]),
    ("ffm_group_train_batch_async_weighted", ctypes.c_int,
     [_vp, ctypes.c_int32] + _CSR + [_vp, ctypes.c_int32]),
    # every stored weight from its accumulators (include/ffm_engine.h "Refresh")
    ("ffm_engine_refresh_weights", ctypes.c_int, [_vp, ctypes.POINTER(RefreshStats)]),
    ("ffm_group_refresh_weights", ctypes.c_int, [_vp, ctypes.POINTER(RefreshStats)]),
    # ids hashed into their field's range (include/ffm_engine.h "Hashed ids")
    ("ffm_engine_hash_ids_device", ctypes.c_int, [_vp, ctypes.c_int32, _vp, _vp, _vp]),
    ("ffm_engine_hash_ids_host", ctypes.c_int,
     [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _i32p, ctypes.c_int32, _i32p, _i32p, _i32p]),
    # weights only, for prediction (include/ffm_engine.h "Serving engines")
    ("ffm_engine_pack_weights", ctypes.c_int, [_vp, _vp, ctypes.POINTER(PackStats)]),
    ("ffm_engine_model_bytes", ctypes.c_int64, [_vp]),
    # one context against many candidates (include/ffm_engine.h "Scoring candidates")
    ("ffm_engine_score_candidates", ctypes.c_int,
     [_vp, ctypes.c_int32, _i32p, _i32p, _i32p, _f32p, _i32p, ctypes.c_int32, _i32p, _i32p, _i32p, _f32p,
      ctypes.c_int32, _f32p]),
    ("ffm_engine_score_candidates_device", ctypes.c_int,
     [_vp, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp, ctypes.c_int32, _vp, _vp, _vp, _vp,
      ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp]),
    # the fields' cardinalities counted on the device, id ranges sized by them (include/ffm_engine.h "Field sketches")
    ("ffm_engine_sketch_create", ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_vp)]),
    ("ffm_engine_sketch_add", ctypes.c_int, [_vp, ctypes.c_int32, _vp, _vp, ctypes.c_int32]),
    ("ffm_engine_sketch_add_device", ctypes.c_int, [_vp, ctypes.c_int32, _vp, _vp]),
    ("ffm_engine_sketch_read", ctypes.c_int, [_vp, _vp, _i64p, _i64p]),
    ("ffm_engine_sketch_destroy", None, [_vp]),
    ("ffm_engine_sketch_estimate", ctypes.c_int, [_vp, ctypes.c_int32, _f64p]),
    ("ffm_engine_field_ranges", ctypes.c_int, [_i64p, ctypes.c_int32, ctypes.c_int32, _i32p]),
    # ids seen fewer than T times share one id per field (include/ffm_engine.h "Rare ids")
    ("ffm_engine_idcount_create", ctypes.c_int,
     [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_vp)]),
    ("ffm_engine_idcount_add", ctypes.c_int, [_vp, ctypes.c_int32, _vp, _vp, ctypes.c_int32]),
    ("ffm_engine_idcount_add_device", ctypes.c_int, [_vp, ctypes.c_int32, _vp, _vp]),
    ("ffm_engine_idcount_read", ctypes.c_int, [_vp, _vp, _i64p, _i64p]),
    ("ffm_engine_idcount_keep", ctypes.c_int, [_vp, ctypes.c_int32, _vp, _i64p, _i64p]),
    ("ffm_engine_idcount_destroy", None, [_vp]),
    ("ffm_engine_set_rare_fold", ctypes.c_int, [_vp, ctypes.c_int32, _vp]),
    ("ffm_engine_sketch_set_filter", ctypes.c_int, [_vp, ctypes.c_int32, _vp]),
    ("ffm_engine_fold_ids_host", ctypes.c_int,
     [ctypes.c_int32, ctypes.c_int32, _vp, ctypes.c_int32, _i32p, _i32p, _i32p]),
    ("ffm_engine_rare_slots_host", ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, _i32p, _i32p, _vp]),
    # numeric fields as quantile buckets (include/ffm_engine.h "Value buckets")
    ("ffm_engine_valhist_create", ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_vp)]),
    ("ffm_engine_valhist_add", ctypes.c_int, [_vp, ctypes.c_int32, _vp, _vp, ctypes.c_int32]),
    ("ffm_engine_valhist_add_device", ctypes.c_int, [_vp, ctypes.c_int32, _vp, _vp]),
    ("ffm_engine_valhist_read", ctypes.c_int, [_vp, _vp, _i64p, _i64p, _i64p]),
    ("ffm_engine_valhist_destroy", None, [_vp]),
    ("ffm_engine_set_buckets", ctypes.c_int, [_vp, _vp, _vp]),
    ("ffm_engine_bucket_ids_device", ctypes.c_int, [_vp, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp]),
    ("ffm_engine_bucket_edges", ctypes.c_int, [_vp, ctypes.c_int32, _vp, ctypes.POINTER(ctypes.c_int32)]),
    ("ffm_engine_bucket_ids_host", ctypes.c_int,
     [ctypes.c_int32, _vp, _vp, ctypes.c_int32, _i32p, _i32p, _f32p, _i32p, _f32p, _vp]),
    # the loss and AUC of the model without each field, in one pass (include/ffm_engine.h "Field ablation")
    ("ffm_engine_ablation_enable", ctypes.c_int, [_vp, ctypes.c_int32]),
    ("ffm_engine_predict_ablated", ctypes.c_int, [_vp, ctypes.c_int32] + _CSR + [ctypes.c_int32, _f32p, _f64p]),
    ("ffm_engine_predict_ablated_device", ctypes.c_int,
     [_vp, ctypes.c_int32, ctypes.c_int32] + _DCSR + [ctypes.c_int32, _vp, _vp]),
    ("ffm_engine_ablation_read", ctypes.c_int, [_vp, ctypes.c_int32, ctypes.POINTER(Metrics)]),
    # the loss and AUC of the model without each field pair, in one pass (include/ffm_engine.h "Pair ablation")
    ("ffm_engine_pair_count", ctypes.c_int32, [ctypes.c_int32]),
    ("ffm_engine_pair_index", ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    ("ffm_engine_pair_fields", ctypes.c_int,
     [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    ("ffm_engine_pair_ablation_enable", ctypes.c_int, [_vp, ctypes.c_int32]),
    ("ffm_engine_predict_pair_ablated", ctypes.c_int, [_vp, ctypes.c_int32] + _CSR + [ctypes.c_int32, _f32p, _f64p]),
    ("ffm_engine_predict_pair_ablated_device", ctypes.c_int,
     [_vp, ctypes.c_int32, ctypes.c_int32] + _DCSR + [ctypes.c_int32, _vp, _vp]),
    ("ffm_engine_pair_ablation_read", ctypes.c_int, [_vp, ctypes.c_int32, ctypes.POINTER(Metrics)]),
    # predict with the kept field pairs only (include/ffm_engine.h "Pair masks")
    ("ffm_engine_set_pair_mask", ctypes.c_int, [_vp, _vp, ctypes.c_int32]),
    ("ffm_engine_get_pair_mask", ctypes.c_int, [_vp, _vp, ctypes.POINTER(ctypes.c_int32)]),
    # the loss and AUC of up to 64 pair masks, in one pass (include/ffm_engine.h "Pruning curve")
    ("ffm_engine_pair_curve_enable", ctypes.c_int, [_vp, _vp, ctypes.c_int32, _i32p, ctypes.c_int32, ctypes.c_int32]),
    ("ffm_engine_predict_pair_curve", ctypes.c_int, [_vp, ctypes.c_int32] + _CSR + [ctypes.c_int32, _f32p, _f64p]),
    ("ffm_engine_predict_pair_curve_device", ctypes.c_int,
     [_vp, ctypes.c_int32, ctypes.c_int32] + _DCSR + [ctypes.c_int32, _vp, _vp]),
    ("ffm_engine_pair_curve_read", ctypes.c_int, [_vp, ctypes.c_int32, ctypes.POINTER(Metrics)]),
    # sync a serving engine, publish only what moved (include/ffm_engine.h "Serving deltas")
    ("ffm_engine_sync_weights", ctypes.c_int, [_vp, _vp, ctypes.POINTER(SyncStats)]),
    ("ffm_engine_sync_moved", ctypes.c_int, [_vp, _i32p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    ("ffm_engine_get_rows_raw", ctypes.c_int, [_vp, ctypes.c_int32, _i32p, _f32p, _vp]),
    ("ffm_engine_set_rows_raw", ctypes.c_int, [_vp, ctypes.c_int32, _i32p, _f32p, _vp]),
    # every row scaled to unit length on the device (include/ffm_engine.h "Normalised rows")
    ("ffm_engine_normalize_rows_device", ctypes.c_int, [_vp, ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp]),
    ("ffm_engine_normalize_rows_host", ctypes.c_int,
     [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _i32p, _i32p, _i32p, _f32p, _f32p]),
    ("ffm_engine_norm_stats", ctypes.c_int, [_vp, ctypes.c_int32, _i64p, _i64p]),
    # libffm / libsvm text parsed on the device (include/ffm_engine.h "Text blocks")
    ("ffm_engine_textparse_create", ctypes.c_int,
     [ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_vp)]),
    ("ffm_engine_textparse_parse", ctypes.c_int, [_vp, ctypes.c_int32, _vp, ctypes.c_int64, ctypes.c_int32]),
    ("ffm_engine_textparse_wait", ctypes.c_int, [_vp, ctypes.c_int32, ctypes.POINTER(TextBlock)]),
    ("ffm_engine_textparse_destroy", None, [_vp]),
    ("ffm_engine_textparse_host", ctypes.c_int,
     [ctypes.c_int32, _vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, _i32p, _i32p, _i32p, _f32p, _i32p,
      ctypes.POINTER(TextBlock)]),
    # blocks cut out of parsed text in HBM and staged from there (include/ffm_engine.h "Resident rows")
    ("ffm_engine_textparse_wait_rows", ctypes.c_int, [_vp, ctypes.c_int32, ctypes.POINTER(TextBlock), ctypes.POINTER(_vp)]),
    ("ffm_engine_rowcut_create", ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_vp)]),
    ("ffm_engine_rowcut_take", ctypes.c_int, [_vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    ("ffm_engine_rowcut_take_host", ctypes.c_int, [_vp, ctypes.c_int32] + _CSR),
    ("ffm_engine_rowcut_close", ctypes.c_int, [_vp, ctypes.POINTER(RowsBlock)]),
    ("ffm_engine_rowcut_release", ctypes.c_int, [_vp, ctypes.c_int32]),
    ("ffm_engine_rowcut_destroy", None, [_vp]),
    ("ffm_engine_stage_batch_resident", ctypes.c_int, [_vp, ctypes.POINTER(RowsBlock)]),
    ("ffm_engine_train_batch_async_resident", ctypes.c_int, [_vp, ctypes.POINTER(RowsBlock)]),
    ("ffm_engine_predict_batch_async_resident", ctypes.c_int, [_vp, ctypes.POINTER(RowsBlock), ctypes.c_int32, _vp]),
]
SKETCH_REGS = 16384  # FFM_SKETCH_REGS
RARE_ID = 2 ** 31 - 1  # FFM_RARE_ID
BUCKET_BINS, BUCKET_MAX_EDGES, BUCKET_NAN_ID = 65536, 255, 65536  # FFM_BUCKET_*
TEXT_MAX_LINE = 65536  # FFM_TEXT_MAX_LINE
# the text kernels' own constants (csrc/kernels_text.h): bytes of a line one wave step reads, bytes per workgroup of
# the newline count, lines per workgroup of the line passes, elements per step of the one-workgroup scans
TEXT_TILE_BYTES, TEXT_SCAN_BYTES, TEXT_LINE_TILE, TEXT_SCAN_CHUNK = 1024, 4096, 64, 256

_lib = None


def default_batch_ramp(w_alpha):
    """The block scheduler's default ramp for a learning rate (ffm_engine_default_batch_ramp)."""
    return int(load_library().ffm_engine_default_batch_ramp(float(w_alpha)))


def shard_plan(n_fields, n_shards, field_map=False):
    """Who owns what under field-pair sharding (ffm_engine_shard_plan): dict(pair_owner [F, F] --
    shard owning the unordered field pair, i.e. both of its latent slots --, lin_owner [F] -- shard
    that adds and updates the linear terms of a field's entries --, bias_owner)."""
    lib = load_library()
    po = np.zeros((n_fields, n_fields), np.int32)
    lo = np.zeros(n_fields, np.int32)
    bo = ctypes.c_int32(0)
    rc = lib.ffm_engine_shard_plan(int(n_fields), int(n_shards), int(bool(field_map)), _i(po), _i(lo),
                                   ctypes.byref(bo))
    if rc != 0:
        raise EngineError(rc, lib.ffm_engine_last_error().decode())
    return dict(pair_owner=po, lin_owner=lo, bias_owner=int(bo.value))


def _channel(channel):
    return _METRIC_CHANNELS[channel] if isinstance(channel, str) else int(channel)


def metrics_from_histogram(pos, neg, n_nan=0):
    """Histogram -> dict(n_pos, n_neg, n_nan, n_mixed_bins, auc, auc_slack) in exact integer
    arithmetic on the host (ffm_engine_metrics_from_histogram: no engine, no device).  pos / neg:
    equally long arrays of counts per score bin, ascending."""
    lib = load_library()
    pos = np.ascontiguousarray(pos, np.uint64)
    neg = np.ascontiguousarray(neg, np.uint64)
    if pos.shape != neg.shape or pos.ndim != 1:
        raise ValueError("pos and neg must be one-dimensional and equally long")
    m = Metrics()
    rc = lib.ffm_engine_metrics_from_histogram(pos.ctypes.data_as(_u64p), neg.ctypes.data_as(_u64p),
                                               pos.size, int(n_nan), ctypes.byref(m))
    if rc != 0:
        raise EngineError(rc, lib.ffm_engine_last_error().decode())
    return m.as_dict()


def metrics_from_keyed(pos, neg, u2):
    """Per-key table -> dict(n_rows, n_keys, n_keys_mixed, n_rows_mixed, n_nan, n_unkeyed, n_overflow, gauc) on the
    host (ffm_engine_metrics_from_keyed: no engine, no device).  pos / neg / u2: P_g, N_g, U2_g of every key,
    keys ascending; the three counters a table does not know come out 0."""
    lib = load_library()
    pos = np.ascontiguousarray(pos, np.int64)
    neg = np.ascontiguousarray(neg, np.int64)
    u2 = np.ascontiguousarray(u2, np.uint64)
    if not (pos.shape == neg.shape == u2.shape) or pos.ndim != 1:
        raise ValueError("pos, neg and u2 must be one-dimensional and equally long")
    m = KeyedMetrics()
    rc = lib.ffm_engine_metrics_from_keyed(pos.ctypes.data_as(_i64p), neg.ctypes.data_as(_i64p), u2.ctypes.data_as(_u64p),
                                           pos.size, ctypes.byref(m))
    if rc != 0:
        raise EngineError(rc, lib.ffm_engine_last_error().decode())
    return m.as_dict()


def keyed_auc_reference(keys, p, labels):
    """The grouped AUC of include/ffm_engine.h "Metrics" (keyed capture) in executable form: numpy integers and
    a Python float loop in the header's order of operations, no library call.  keys: one int per row, negative
    = the row has no key (counted in n_unkeyed); p: float32 scores, NaN rows counted in n_nan; labels: positive
    iff > 0.  Returns the dict Engine.metrics_read_keyed returns (n_overflow 0) plus the table "key", "pos",
    "neg", "u2" (int64 / int64 / int64 / uint64 arrays, keys ascending)."""
    keys = np.asarray(keys, np.int64).reshape(-1)
    p = np.asarray(p, np.float32).reshape(-1)
    y = np.asarray(labels).reshape(-1) > 0
    if not (keys.shape == p.shape == y.shape):
        raise ValueError("keys, p and labels must be equally long")
    nan = np.isnan(p)
    unkeyed = ~nan & (keys < 0)
    ok = ~nan & ~unkeyed
    k, s, y = keys[ok], p[ok].astype(np.float64), y[ok]
    order = np.lexsort((y, s, k))  # key, then score, negatives first inside a tie
    k, s, y = k[order], s[order], y[order]
    n = k.size
    idx = np.arange(n, dtype=np.int64)
    key_start = np.ones(n, bool)
    key_start[1:] = k[1:] != k[:-1]
    run_start = key_start.copy()
    run_start[1:] |= s[1:] != s[:-1]
    neg_before = np.cumsum(~y) - (~y)                       # negatives in [0, i)
    at_key = neg_before[np.maximum.accumulate(np.where(key_start, idx, 0))] if n else neg_before
    at_run = neg_before[np.maximum.accumulate(np.where(run_start, idx, 0))] if n else neg_before
    contrib = np.where(y, 2 * (neg_before - at_key) - (neg_before - at_run), 0).astype(np.int64)
    g = np.cumsum(key_start) - 1                            # the row's key number
    n_keys = int(g[-1]) + 1 if n else 0
    pos = np.bincount(g[y], minlength=n_keys).astype(np.int64)
    neg = np.bincount(g[~y], minlength=n_keys).astype(np.int64)
    u2 = np.zeros(n_keys, np.int64)
    np.add.at(u2, g, contrib)
    num = den = 0.0
    n_mixed = rows_mixed = 0
    for P, N, U in zip(pos.tolist(), neg.tolist(), u2.tolist()):
        if P == 0 or N == 0:
            continue
        auc_g = float(U) / (2.0 * float(P) * float(N))
        num += float(P + N) * auc_g
        den += float(P + N)
        n_mixed += 1
        rows_mixed += P + N
    return dict(n_rows=int(n), n_keys=n_keys, n_keys_mixed=n_mixed, n_rows_mixed=rows_mixed, n_nan=int(nan.sum()),
                n_unkeyed=int(unkeyed.sum()), n_overflow=0, gauc=num / den if den else float("nan"),
                key=k[key_start].astype(np.int64), pos=pos, neg=neg, u2=u2.astype(np.uint64))


def init_weights_host(seed, mean, stddev, latent, first, count):
    """The weights a fresh engine holds, recomputed on the host (ffm_engine_init_weights_host)."""
    out = np.empty(int(count), np.float32)
    rc = load_library().ffm_engine_init_weights_host(int(seed), mean, stddev, int(bool(latent)),
                                                     int(first), int(count), _f(out))
    if rc != 0:
        raise EngineError(rc, load_library().ffm_engine_last_error().decode())
    return out


def hash_ids(field, feat, n_feats, field_start=None, model="ffm", n_fields=None):
    """The model ids a flagged engine (hash_ids=True) gives raw ids, computed on the host
    (ffm_engine_hash_ids_host: the device's bits, no device needed).  field: the entries' fields, or None
    (LR / FM have none; FFM: rows of one entry per field in field order, n_fields needed).  field_start:
    the fields' id ranges the engine was given, or None = one range [0, n_feats).  n_fields: fields outside
    [0, n_fields) erase their entry (id -1); default len(field_start) - 1, else every field >= 0 is valid."""
    lib = load_library()
    mt = MODEL_TYPES[model.upper()] if isinstance(model, str) else int(model)
    feat = np.ascontiguousarray(feat, np.int32)
    fld = None if field is None or mt != FFM else np.ascontiguousarray(field, np.int32)
    fs = None if field_start is None or mt != FFM else np.ascontiguousarray(field_start, np.int32)
    if n_fields is None:
        if fs is None and fld is None and mt == FFM:
            raise ValueError("FFM rows without a field array need n_fields")
        n_fields = fs.size - 1 if fs is not None else 2 ** 31 - 1
    if fld is not None and fld.shape != feat.shape:
        raise ValueError("field and feat must be equally long")
    out = np.empty_like(feat)
    rc = lib.ffm_engine_hash_ids_host(mt, int(n_feats), int(n_fields), _i(fs), feat.size, _i(fld), _i(feat), _i(out))
    if rc != 0:
        raise EngineError(rc, lib.ffm_engine_last_error().decode())
    return out


def _norm_args(row_ptr, field, feat, val, n_fields, model):
    """normalize_rows / normalize_rows_host: the arrays as int32 / float32 and the model type, checked."""
    mt = MODEL_TYPES[model.upper()] if isinstance(model, str) else int(model)
    row_ptr = np.ascontiguousarray(row_ptr, np.int32)
    feat = np.ascontiguousarray(feat, np.int32)
    fld = None if field is None or mt != FFM else np.ascontiguousarray(field, np.int32)
    val = None if val is None else np.ascontiguousarray(val, np.float32)
    if mt == FFM and n_fields is None:
        raise ValueError("FFM needs n_fields")
    if row_ptr.ndim != 1 or row_ptr.size < 1 or row_ptr[0] != 0 or np.any(np.diff(row_ptr) < 0) or row_ptr[-1] != feat.size:
        raise ValueError("row_ptr must ascend from 0 to len(feat)")
    if (fld is not None and fld.shape != feat.shape) or (val is not None and val.shape != feat.shape):
        raise ValueError("field, feat and val must be equally long")
    return mt, row_ptr, fld, feat, val


def normalize_rows(row_ptr, field, feat, val, n_feats, n_fields=None, model="ffm"):
    """What an engine created with normalize=True makes of a block's values (include/ffm_engine.h "Normalised
    rows"), in numpy: per row s = fl(s + fl(v * v)) over the kept entries in entry order (0 <= feat < n_feats;
    FFM with a field array also 0 <= field < n_fields), scale = fl(1 / fl(sqrt(s))) where s > 0 and finite, else
    the row stays as it came; every entry of the row, kept or not, becomes fl(v * scale).  np.float32 scalars
    throughout: one rounding per operation, sequential on purpose.  val None: ones.  Returns a new float32 array."""
    mt, row_ptr, fld, feat, val = _norm_args(row_ptr, field, feat, val, n_fields, model)
    out = np.ones(feat.size, np.float32) if val is None else val.copy()
    keep = (feat >= 0) & (feat < int(n_feats))
    if fld is not None:
        keep &= (fld >= 0) & (fld < int(n_fields))
    one, inf = np.float32(1.0), np.float32(np.inf)
    with np.errstate(all="ignore"):
        for r in range(row_ptr.size - 1):
            b, e = int(row_ptr[r]), int(row_ptr[r + 1])
            s = np.float32(0.0)
            for p in range(b, e):
                if keep[p]:
                    s = np.float32(s + np.float32(out[p] * out[p]))
            if s > 0 and s < inf:
                scale = np.float32(one / np.float32(np.sqrt(s)))
                for p in range(b, e):
                    out[p] = np.float32(out[p] * scale)
    return out


def normalize_rows_host(row_ptr, field, feat, val, n_feats, n_fields=None, model="ffm"):
    """normalize_rows by the library's plain C++ twin (ffm_engine_normalize_rows_host: the kernel's bits, no
    device needed)."""
    lib = load_library()
    mt, row_ptr, fld, feat, val = _norm_args(row_ptr, field, feat, val, n_fields, model)
    out = np.empty(feat.size, np.float32)
    rc = lib.ffm_engine_normalize_rows_host(mt, int(n_feats), int(n_fields or 0), row_ptr.size - 1, _i(row_ptr), _i(fld), _i(feat),
                                            _f(val), _f(out))
    if rc != 0:
        raise EngineError(rc, lib.ffm_engine_last_error().decode())
    return out


def _rare_words(bits, words):
    """A keep-map as the library takes it: uint64 [2^bits / 64], contiguous."""
    bits = int(bits)
    if not 8 <= bits <= 30:
        raise ValueError("bits must lie in [8, 30]")
    words = np.ascontiguousarray(words, np.uint64)
    if words.shape != ((1 << bits) // 64,):
        raise ValueError("words: uint64 [2^bits / 64] = [%d]" % ((1 << bits) // 64))
    return bits, words


def rare_slot(field, feat, bits):
    """The slot of every entry (uint32): the top `bits` of its hashed bits, what an IdCounter counts and a
    keep-map tests (ffm_engine_rare_slots_host: no device).  field None: LR / FM, the field is taken as 0."""
    lib = load_library()
    feat = np.ascontiguousarray(feat, np.int32)
    fld = None if field is None else np.ascontiguousarray(field, np.int32)
    if fld is not None and fld.shape != feat.shape:
        raise ValueError("field and feat must be equally long")
    out = np.zeros(feat.shape, np.uint32)
    rc = lib.ffm_engine_rare_slots_host(int(bits), feat.size, _i(fld), _i(feat), out.ctypes.data)
    if rc != 0:
        raise EngineError(rc, lib.ffm_engine_last_error().decode())
    return out


def fold_rare(field, feat, n_fields, bits, words):
    """The raw ids an engine with the keep-map `words` hashes (ffm_engine_fold_ids_host: the device's bits, no
    device): RARE_ID where a counting entry's bit is 0, feat elsewhere.  n_fields 0: LR / FM (field ignored);
    field None with n_fields > 0: entry p is field p mod n_fields.  hash_ids of the result gives the model ids."""
    lib = load_library()
    bits, words = _rare_words(bits, words)
    feat = np.ascontiguousarray(feat, np.int32)
    fld = None if field is None or int(n_fields) == 0 else np.ascontiguousarray(field, np.int32)
    if fld is not None and fld.shape != feat.shape:
        raise ValueError("field and feat must be equally long")
    out = np.empty_like(feat)
    rc = lib.ffm_engine_fold_ids_host(int(n_fields), bits, words.ctypes.data, feat.size, _i(fld), _i(feat), _i(out))
    if rc != 0:
        raise EngineError(rc, lib.ffm_engine_last_error().decode())
    return out


def value_bins(val):
    """(bin int32, is_nan bool) of float32 values (include/ffm_engine.h "Value buckets"): the top 16 bits of the
    order-preserving key of every value's bit pattern; a NaN has no bin (-1 here).  Integer arithmetic only."""
    u = np.ascontiguousarray(val, np.float32).view(np.uint32).copy()
    u[(u & np.uint32(0x7fffffff)) == 0] = 0
    nan = (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    key = np.where((u >> np.uint32(31)) != 0, ~u, u | np.uint32(0x80000000))
    bins = (key >> np.uint32(16)).astype(np.int32)
    bins[nan] = -1
    return bins, nan


def bucket_edges(counts, n_buckets):
    """The edges (uint16, strictly ascending, at most BUCKET_MAX_EDGES) that cut one field's value histogram
    (BUCKET_BINS counts) into n_buckets buckets of equal mass (ffm_engine_bucket_edges: exact integers, no device)."""
    lib = load_library()
    counts = np.ascontiguousarray(counts, np.uint64)
    if counts.shape != (BUCKET_BINS,):
        raise ValueError("counts: uint64 [%d]" % BUCKET_BINS)
    edges = np.zeros(BUCKET_MAX_EDGES, np.uint16)
    n = ctypes.c_int32(0)
    rc = lib.ffm_engine_bucket_edges(counts.ctypes.data, int(n_buckets), edges.ctypes.data, ctypes.byref(n))
    if rc != 0:
        raise EngineError(rc, lib.ffm_engine_last_error().decode())
    return edges[:n.value].copy()


def _bucket_table(n_fields, buckets):
    """{field: edges} as the library takes a table: (n_edges int32 [n_fields], edges uint16 [n_fields, 255])."""
    n_fields = int(n_fields)
    n_edges = np.full(n_fields, -1, np.int32)
    edges = np.zeros((max(n_fields, 1), BUCKET_MAX_EDGES), np.uint16)
    for f, e in buckets.items():
        f = int(f)
        if not 0 <= f < n_fields:
            raise ValueError("bucketed field %d outside [0, %d)" % (f, n_fields))
        e = np.asarray(e)
        if e.ndim != 1 or e.size > BUCKET_MAX_EDGES or (e.size and (e.min() < 0 or e.max() >= BUCKET_BINS)):
            raise ValueError("field %d: at most %d edges, each a bin in [0, %d)" % (f, BUCKET_MAX_EDGES, BUCKET_BINS))
        n_edges[f] = e.size
        edges[f, :e.size] = e.astype(np.uint16)
    return n_edges, edges


def bucket_ids(field, feat, val, n_fields, buckets):
    """The bucket step of an engine with the table `buckets` = {field: edges} on the host
    (ffm_engine_bucket_ids_host: the device's bits, no device): (feat', val', bucketed bool).  A bucketed entry is
    (bucket, 1.0); every other entry comes back untouched.  field None: entry p is field p mod n_fields; val None:
    every value is 1.0."""
    lib = load_library()
    n_edges, edges = _bucket_table(n_fields, buckets)
    feat = np.ascontiguousarray(feat, np.int32)
    fld = None if field is None else np.ascontiguousarray(field, np.int32)
    v = None if val is None else np.ascontiguousarray(val, np.float32)
    if (fld is not None and fld.shape != feat.shape) or (v is not None and v.shape != feat.shape):
        raise ValueError("field, feat and val must be equally long")
    feat_out, val_out, hit = np.empty_like(feat), np.empty(feat.shape, np.float32), np.zeros(feat.shape, np.uint8)
    rc = lib.ffm_engine_bucket_ids_host(int(n_fields), n_edges.ctypes.data, edges.ctypes.data, feat.size, _i(fld), _i(feat),
                                        _f(v), _i(feat_out), _f(val_out), hit.ctypes.data)
    if rc != 0:
        raise EngineError(rc, lib.ffm_engine_last_error().decode())
    return feat_out, val_out, hit.astype(bool)


def sketch_estimate(reg):
    """Distinct ids per field from a sketch's registers (uint8 [n_fields, SKETCH_REGS]), float64 [n_fields]
    (ffm_engine_sketch_estimate: host arithmetic, no device)."""
    lib = load_library()
    reg = np.ascontiguousarray(reg, np.uint8)
    if reg.ndim != 2 or reg.shape[1] != SKETCH_REGS:
        raise ValueError("reg: uint8 [n_fields, %d]" % SKETCH_REGS)
    out = np.zeros(reg.shape[0], np.float64)
    rc = lib.ffm_engine_sketch_estimate(reg.ctypes.data, reg.shape[0], out.ctypes.data_as(_f64p))
    if rc != 0:
        raise EngineError(rc, lib.ffm_engine_last_error().decode())
    return out


def field_ranges(count, n_feats):
    """field_start (int32 [n_fields + 1]) for per-field counts of distinct ids: every field's share of n_feats
    in proportion to its count above a floor (ffm_engine_field_ranges: exact integers, no device)."""
    lib = load_library()
    count = np.ascontiguousarray(count, np.int64)
    if count.ndim != 1:
        raise ValueError("count: one integer per field")
    out = np.zeros(count.size + 1, np.int32)
    rc = lib.ffm_engine_field_ranges(count.ctypes.data_as(_i64p), count.size, int(n_feats), _i(out))
    if rc != 0:
        raise EngineError(rc, lib.ffm_engine_last_error().decode())
    return out


def drop_field(block, f):
    """The block without every entry whose field is f (include/ffm_engine.h "Field ablation"): rows, labels and
    the order of the remaining entries stay as they are; val may be None."""
    from .synth import Block
    field = np.asarray(block.field)
    keep = field != f
    kept = np.concatenate(([0], np.cumsum(keep, dtype=np.int64)))
    row_ptr = kept[np.asarray(block.row_ptr, np.int64)].astype(np.int32)
    return Block(row_ptr, np.ascontiguousarray(field[keep], np.int32), np.ascontiguousarray(np.asarray(block.feat)[keep], np.int32),
                 None if block.val is None else np.ascontiguousarray(np.asarray(block.val)[keep], np.float32), block.label)


def pair_count(n_fields):
    """V = n_fields (n_fields + 1) / 2: the unordered field pairs with the diagonal (include/ffm_engine.h "Pair
    ablation"; host arithmetic, no device).  n_fields in 1 .. 64."""
    lib = load_library()
    v = lib.ffm_engine_pair_count(int(n_fields))
    if v < 0:
        raise EngineError(E_INVALID, lib.ffm_engine_last_error().decode())
    return int(v)


def pair_index(n_fields, f, g):
    """The variant of the pair {f, g}, in either order: for f <= g, f * F - f * (f - 1) / 2 + (g - f)."""
    lib = load_library()
    v = lib.ffm_engine_pair_index(int(n_fields), int(f), int(g))
    if v < 0:
        raise EngineError(E_INVALID, lib.ffm_engine_last_error().decode())
    return int(v)


def pair_fields(n_fields, v):
    """(f, g) with f <= g and pair_index(n_fields, f, g) == v, for v in [0, pair_count(n_fields))."""
    lib = load_library()
    f, g = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = lib.ffm_engine_pair_fields(int(n_fields), int(v), ctypes.byref(f), ctypes.byref(g))
    if rc != 0:
        raise EngineError(rc, lib.ffm_engine_last_error().decode())
    return int(f.value), int(g.value)


def drop_pair_weights(vec_w, ids_of_field_f, g):
    """A copy of vec_w [n_feats, n_fields, k] (a 2-d table: vec_w.reshape(n_feats, n_fields, k)) with the slot
    "towards field g" set to +0.0 for every id in ids_of_field_f: the weights on which predict_batch gives
    variant (f, g) of pair ablation bit for bit (include/ffm_engine.h "Pair ablation", "as weights"; f == g
    zeroes the field's own slot).  Two conditions, both the caller's: every feature id of the block occurs under
    one field only (else the zeroed slot also removes terms of another pair), and the model's bias is not -0.0 (a
    running sum that starts anywhere else is never -0.0, so adding the +-0.0 such a term becomes changes no bit)."""
    w = np.array(vec_w, np.float32, copy=True)
    if w.ndim != 3:
        raise ValueError("vec_w: [n_feats, n_fields, k] (reshape a 2-d table first)")
    ids = np.asarray(ids_of_field_f, np.int64).reshape(-1)
    w[ids, int(g), :] = np.float32(0.0)
    return w


def pair_mask(n_fields, kept_pairs):
    """keep[n_fields] (uint64) of a pair mask (include/ffm_engine.h "Pair masks") from the kept pairs (f, g), each in
    either order, (f, f) the diagonal: bit g of keep[f] and bit f of keep[g] -- symmetric by construction."""
    n_fields = int(n_fields)
    if n_fields < 1 or n_fields > 64:
        raise ValueError("a pair mask is for 1 .. 64 fields, got n_fields = %d" % n_fields)
    words = [0] * n_fields
    for f, g in kept_pairs:
        f, g = int(f), int(g)
        if f < 0 or g < 0 or f >= n_fields or g >= n_fields:
            raise ValueError("pair (%d, %d) names a field outside [0, %d)" % (f, g, n_fields))
        words[f] |= 1 << g
        words[g] |= 1 << f
    return np.array(words, np.uint64)


def pair_mask_pairs(words):
    """The kept pairs of a mask, sorted (f, g) with f <= g: pair_mask's inverse.  An asymmetric mask or a bit at or
    above the number of words is a ValueError."""
    w = [int(x) for x in np.asarray(words, np.uint64).reshape(-1)]
    n = len(w)
    if n < 1 or n > 64:
        raise ValueError("a pair mask is for 1 .. 64 fields, got %d words" % n)
    pairs = []
    for f in range(n):
        if w[f] >> n:
            raise ValueError("keep[%d] has a bit at or above n_fields = %d" % (f, n))
        for g in range(n):
            if (w[f] >> g) & 1 != (w[g] >> f) & 1:
                raise ValueError("the mask is not symmetric in (%d, %d)" % (f, g))
            if g >= f and (w[f] >> g) & 1:
                pairs.append((f, g))
    return pairs


def pair_mask_top(n_fields, loss, n_keep):
    """The mask of the n_keep pairs whose removal costs most.  loss[V + 1] as predict_pair_ablated sums it (V =
    pair_count(n_fields)): loss[v] the loss without pair v, loss[V] the loss of the rows.  The pairs are ranked by
    delta = loss[v] - loss[V], largest first, ties to the lower pair index; the first n_keep are kept (0 <= n_keep
    <= V).  A delta that is not finite is a ValueError: "pair mask: loss without pair f g is not finite"."""
    V = pair_count(n_fields)
    loss = np.asarray(loss, np.float64).reshape(-1)
    if loss.shape[0] != V + 1:
        raise ValueError("loss: one sum per pair and the rows' own, %d in all, got %d" % (V + 1, loss.shape[0]))
    n_keep = int(n_keep)
    if n_keep < 0 or n_keep > V:
        raise ValueError("n_keep must lie in [0, %d], got %d" % (V, n_keep))
    with np.errstate(invalid="ignore", over="ignore"):
        delta = loss[:V] - loss[V]
    bad = np.flatnonzero(~np.isfinite(delta))
    if bad.size:
        raise ValueError("pair mask: loss without pair %d %d is not finite" % pair_fields(n_fields, int(bad[0])))
    order = sorted(range(V), key=lambda v: -delta[v])  # (stable: ties stay in index order)
    return pair_mask(n_fields, [pair_fields(n_fields, v) for v in sorted(order[:n_keep])])


def pair_curve_levels(n_fields, order):
    """The level table of a ladder (include/ffm_engine.h "Pruning curve"): order is a permutation of the V =
    n_fields (n_fields + 1) / 2 pair indices, best first; level[f][g] = level[g][f] = the position of pair (f, g) in
    it, so that cut N keeps the best N pairs.  uint16[n_fields, n_fields].  Pure numpy."""
    n_fields = int(n_fields)
    if n_fields < 1 or n_fields > 64:
        raise ValueError("a level table is for 1 .. 64 fields, got n_fields = %d" % n_fields)
    V = n_fields * (n_fields + 1) // 2
    order = np.asarray(order, np.int64).reshape(-1)
    if order.shape[0] != V or not np.array_equal(np.sort(order), np.arange(V)):
        raise ValueError("order must be a permutation of the %d pair indices of %d fields" % (V, n_fields))
    rank = np.empty(V, np.int64)
    rank[order] = np.arange(V)
    f, g = np.triu_indices(n_fields)  # (row-major over f <= g: the pairs in pair_index order)
    level = np.zeros((n_fields, n_fields), np.uint16)
    level[f, g] = rank
    level[g, f] = rank
    return level


def pair_curve_mask(level, cut):
    """The mask that one cut of a level table stands for, in pair_mask's format: bit g of words[f] is
    level[f][g] < cut (include/ffm_engine.h "Pruning curve", "as masks").  Pure numpy."""
    level = np.asarray(level)
    if level.ndim != 2 or level.shape[0] != level.shape[1] or not 1 <= level.shape[0] <= 64:
        raise ValueError("level: a square table of 1 .. 64 fields")
    if level.dtype.kind not in "ui" or level.min() < 0 or level.max() > 65535:
        raise ValueError("level: unsigned 16-bit entries")
    if not np.array_equal(level, level.T):
        raise ValueError("the level table is not symmetric")
    cut = int(cut)
    if cut < 0 or cut > 65536:
        raise ValueError("a cut lies in [0, 65536], got %d" % cut)
    kept = level.astype(np.int64) < cut
    bit = np.uint64(1) << np.arange(level.shape[0], dtype=np.uint64)
    return (kept.astype(np.uint64) * bit[None, :]).sum(axis=1, dtype=np.uint64)


def spell_out_candidates(ctx, cand_req_ptr, cand):
    """The block of rows [context entries ..., candidate entries ...] that Engine.score_candidates scores:
    row c is the context of candidate c's request followed by the candidate's own entries (include/ffm_engine.h
    "Scoring candidates" in executable form; numpy only).  ctx: one row per request; cand_req_ptr[n_req + 1]:
    the candidates of request r are rows [cand_req_ptr[r], cand_req_ptr[r + 1]) of cand.  A val of None reads as
    ones; the result always carries its values, and labels of 0."""
    from .synth import Block
    cand_req_ptr = np.asarray(cand_req_ptr, np.int64)
    n_req, n_cand = ctx.n_rows, cand.n_rows
    if cand_req_ptr.shape != (n_req + 1,) or cand_req_ptr[0] != 0 or cand_req_ptr[-1] != n_cand or (np.diff(cand_req_ptr) < 0).any():
        raise ValueError("cand_req_ptr must ascend from 0 to the number of candidates, one step per request")
    req = np.repeat(np.arange(n_req, dtype=np.int64), np.diff(cand_req_ptr))  # the request of every candidate
    cp, kp = np.asarray(ctx.row_ptr, np.int64), np.asarray(cand.row_ptr, np.int64)
    n_ctx, n_own = np.diff(cp)[req], np.diff(kp)
    row_ptr = np.concatenate([[0], np.cumsum(n_ctx + n_own)])
    nnz = int(row_ptr[-1])
    row = np.repeat(np.arange(n_cand, dtype=np.int64), n_ctx + n_own)   # the row of every output entry
    at = np.arange(nnz, dtype=np.int64) - row_ptr[row]                 # its position in that row
    from_ctx = at < n_ctx[row]
    src = np.where(from_ctx, cp[req[row]] + at, kp[row] + at - n_ctx[row])

    def merged(a, b, dtype):
        a = np.ones(int(cp[-1]), dtype) if a is None else np.asarray(a, dtype)
        b = np.ones(int(kp[-1]), dtype) if b is None else np.asarray(b, dtype)
        out = np.empty(nnz, dtype)
        out[from_ctx] = a[src[from_ctx]]
        out[~from_ctx] = b[src[~from_ctx]]
        return out
    return Block(row_ptr.astype(np.int32), merged(ctx.field, cand.field, np.int32), merged(ctx.feat, cand.feat, np.int32),
                 merged(ctx.val, cand.val, np.float32), np.zeros(n_cand, np.int32))


def load_library(path=None):
    """dlopen libffm_engine.so and bind every ABI symbol.  Raises if it is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or os.environ.get("FFM_ENGINE_LIB") or LIB_PATH  # env: A/B experiments only
    if not os.path.exists(path):
        raise FileNotFoundError(
            "%s not found: build it with `python ftrl-ffm_amd/build.py` (hipcc, gfx950). "
            "There is no CPU fallback." % path)
    lib = ctypes.CDLL(path)
    for name, restype, argtypes in ABI:
        fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def page_aligned(n, dtype):
    """A numpy array of n elements in an anonymous mapping of its own: page-aligned, whole pages,
    shared with nothing else -- what Engine.pin_block should be given.  (hipHostRegister locks whole
    pages; an array in the middle of the Python heap shares its pages with whatever lives next to
    it, and the runtime then meets half-registered ranges in later copies.)"""
    import mmap
    nbytes = max(1, int(n)) * np.dtype(dtype).itemsize
    size = (nbytes + mmap.PAGESIZE - 1) // mmap.PAGESIZE * mmap.PAGESIZE
    return np.frombuffer(mmap.mmap(-1, size), dtype=dtype, count=int(n))


def _f(a):
    return None if a is None else a.ctypes.data_as(_f32p)


def _i(a):
    return None if a is None else a.ctypes.data_as(_i32p)


def _w(weight, n_rows):
    """A block's sample weights as the address the *_weighted entry points take: a contiguous float32
    array of at least n_rows elements (the caller keeps it alive; a zero_copy one page-locked)."""
    if weight.dtype != np.float32 or weight.ndim != 1 or weight.size < n_rows or not weight.flags.c_contiguous:
        raise ValueError("weight: a contiguous float32 array of at least n_rows elements")
    return weight.ctypes.data


STATE_KEYS = ("bias3", "lin_w", "lin_n", "lin_z", "vec_w", "vec_n", "vec_z")


class Engine:
    """One LR / FM / FFM model resident in HBM (mirrors ftrl::FtrlModel for blocks of rows)."""

    def __init__(self, model_type="FFM", n_feats=10000, n_fields=8, n_factors=16, w_alpha=1e-4,
                 w_beta=1.0, w_l1=0.1, w_l2=5.0, init_mean=0.0, init_stddev=0.02, seed=42,
                 max_batch_rows=8192, max_batch_nnz=None, device_id=0, n_shards=1, shard_rank=0,
                 stream=None, skip_init=False, max_row_nnz=0, learn=False, field_start=None, hash_ids=False,
                 serve=None, normalize=False):
        """normalize: every row handed over in host memory is scaled to unit Euclidean length on the device before
        any kernel reads its values (include/ffm_engine.h "Normalised rows"; normalize_rows is the same on the host).
        serve: None = a training engine; "f32" / "f16" = a serving engine (include/ffm_engine.h "Serving
        engines"): bias, lin_w and a latent table of w alone in fp32 bits or IEEE binary16 -- prediction only."""
        self.lib = load_library()
        if serve not in SERVE_FLAGS:
            raise ValueError("serve: None, 'f32' or 'f16'")
        self.serve = serve if SERVE_FLAGS[serve] else None
        cfg = Config()
        self.lib.ffm_engine_default_config(ctypes.byref(cfg))
        cfg.model_type = MODEL_TYPES[model_type] if isinstance(model_type, str) else int(model_type)
        cfg.n_feats, cfg.n_fields, cfg.n_factors = int(n_feats), int(n_fields), int(n_factors)
        cfg.w_alpha, cfg.w_beta, cfg.w_l1, cfg.w_l2 = w_alpha, w_beta, w_l1, w_l2
        cfg.init_mean, cfg.init_stddev, cfg.seed = init_mean, init_stddev, int(seed)
        cfg.max_batch_rows = int(max_batch_rows)
        cfg.max_batch_nnz = int(max_batch_nnz if max_batch_nnz else max_batch_rows * 64)
        cfg.device_id, cfg.n_shards, cfg.shard_rank = int(device_id), int(n_shards), int(shard_rank)
        cfg.stream = stream
        cfg.flags = ((FLAG_SKIP_INIT if skip_init else 0) | (FLAG_LEARN if learn else 0) | (FLAG_HASH_IDS if hash_ids else 0)
                     | SERVE_FLAGS[serve] | (FLAG_NORM_ROWS if normalize else 0))
        cfg.max_row_nnz = int(max_row_nnz)
        self._field_start = None
        if field_start is not None:
            self._field_start = np.ascontiguousarray(field_start, np.int32)
            cfg.field_start = _i(self._field_start)
        self.cfg = cfg
        self.h = _vp()
        self._check(self.lib.ffm_engine_create(ctypes.byref(cfg), ctypes.byref(self.h)))
        self.model_type = cfg.model_type
        self.n_feats, self.n_fields, self.n_factors = cfg.n_feats, cfg.n_fields, cfg.n_factors
        self.row_len = int(self.lib.ffm_engine_row_len(self.h))

    def _check(self, rc):
        if rc != 0:
            raise EngineError(rc, self.lib.ffm_engine_last_error().decode())

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.ffm_engine_destroy(self.h)
            self.h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- state ----
    def zero_state(self):
        nf, L = self.n_feats, self.row_len
        return dict(bias3=np.zeros(3, np.float32), lin_w=np.zeros(nf, np.float32),
                    lin_n=np.zeros(nf, np.float32), lin_z=np.zeros(nf, np.float32),
                    vec_w=np.zeros((nf, L), np.float32), vec_n=np.zeros((nf, L), np.float32),
                    vec_z=np.zeros((nf, L), np.float32))

    def get_weights(self):
        """dict(bias, lin_w, vec_w): the weights alone (a serving engine: its table decoded to fp32)."""
        b = np.zeros(1, np.float32)
        lw = np.zeros(self.n_feats, np.float32)
        vw = np.zeros((self.n_feats, self.row_len), np.float32)
        self._check(self.lib.ffm_engine_get_weights(self.h, _f(b), _f(lw), _f(vw) if self.row_len else None))
        return dict(bias=b, lin_w=lw, vec_w=vw)

    def set_weights(self, bias=None, lin_w=None, vec_w=None):
        """Overwrites the given weights (fp32 host arrays; a serving engine rounds vec_w to its format)."""
        c = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)  # noqa: E731
        b, lw, vw = c(bias), c(lin_w), c(vec_w)
        self._check(self.lib.ffm_engine_set_weights(self.h, _f(b.reshape(-1)[:1].copy()) if b is not None else None,
                                                    _f(lw), _f(vw) if vw is not None and vw.size else None))

    def model_bytes(self):
        """Bytes of HBM requested for the model arrays: bias, linear, latent (ffm_engine_model_bytes)."""
        return int(self.lib.ffm_engine_model_bytes(self.h))

    def pack_from(self, src):
        """This serving engine's weights from a training engine of the same shape on the same device, in one
        device pass (ffm_engine_pack_weights): src's STORED bias, lin_w and w -- src.refresh_weights() first
        when the learned model is wanted.  Returns dict(n_latent, n_inexact, n_to_inf, n_to_zero)."""
        st = PackStats()
        self._check(self.lib.ffm_engine_pack_weights(self.h, src.h, ctypes.byref(st)))
        return st.as_dict()

    # ---- serving deltas (include/ffm_engine.h "Serving deltas") ----
    def sync_from(self, src):
        """pack_from(src) by comparison (ffm_engine_sync_weights): afterwards this serving engine holds, bit for
        bit, what pack_from(src) would have left, but only the features whose patterns differed were written, and
        their set stays on the device for sync_moved().  Returns dict(n_moved, n_lin_moved, n_lat_moved, bias_moved)."""
        st = SyncStats()
        self._check(self.lib.ffm_engine_sync_weights(self.h, src.h, ctypes.byref(st)))
        return st.as_dict()

    def sync_moved(self):
        """Ascending int32 ids of the features the last sync_from() moved (ffm_engine_sync_moved)."""
        n = ctypes.c_int64(0)
        self._check(self.lib.ffm_engine_sync_moved(self.h, None, 0, ctypes.byref(n)))
        ids = np.empty(n.value, np.int32)
        self._check(self.lib.ffm_engine_sync_moved(self.h, _i(ids), ids.size, ctypes.byref(n)))
        return ids[:n.value]

    def _raw_dtype(self):
        if not self.serve:
            raise EngineError(E_UNSUPPORTED, "raw rows are a serving engine's: a training engine has get_rows / set_rows")
        return RAW_DTYPES[self.serve]

    def get_rows_raw(self, ids):
        """The listed features as this serving engine stores them (ffm_engine_get_rows_raw): (lin_w float32 [n],
        lat [n, row_len] of np.float32 (f32) or np.uint16 (f16: the halves' bits)); no conversion."""
        ids = np.ascontiguousarray(ids, np.int32)
        lw = np.zeros(ids.size, np.float32)
        lat = np.zeros((ids.size, self.row_len), RAW_DTYPES.get(self.serve, np.float32))
        self._check(self.lib.ffm_engine_get_rows_raw(self.h, ids.size, _i(ids), _f(lw), lat.ctypes.data if lat.size else None))
        return lw, lat

    def set_rows_raw(self, ids, lin_w=None, lat=None):
        """Overwrites the listed features' lin_w and / or rows with the given bits (ffm_engine_set_rows_raw);
        lat: [n, row_len] of the format's own dtype (np.float32 / np.uint16), taken as it is."""
        ids = np.ascontiguousarray(ids, np.int32)
        lw = None if lin_w is None else np.ascontiguousarray(lin_w, np.float32)
        if lw is not None and lw.size != ids.size:
            raise ValueError("lin_w: one float32 per id")
        if lat is not None:
            dt = RAW_DTYPES.get(self.serve, np.float32)
            lat = np.ascontiguousarray(lat)
            if lat.dtype != dt or lat.size != ids.size * self.row_len:
                raise ValueError("lat: [n, row_len] of %s" % np.dtype(dt).name)
        self._check(self.lib.ffm_engine_set_rows_raw(self.h, ids.size, _i(ids), _f(lw),
                                                     lat.ctypes.data if lat is not None and lat.size else None))

    def export_delta(self):
        """What the last sync_from() moved, in this engine's own bits: dict(fmt, ids, bias, lin_w, lat).
        apply_delta() of it on an engine that held what this one held before that sync reproduces this one."""
        self._raw_dtype()
        ids = self.sync_moved()
        lw, lat = self.get_rows_raw(ids)
        b = np.zeros(1, np.float32)
        self._check(self.lib.ffm_engine_get_weights(self.h, _f(b), None, None))
        return dict(fmt=self.serve, ids=ids, bias=b, lin_w=lw, lat=lat)

    def apply_delta(self, d):
        """set_rows_raw of an export_delta() plus its bias; refuses a fmt or row_len that is not this engine's."""
        dt = self._raw_dtype()
        ids = np.ascontiguousarray(d["ids"], np.int32)
        lat = np.asarray(d["lat"])
        if d["fmt"] != self.serve or lat.dtype != dt:
            raise EngineError(E_INVALID, "apply_delta: a delta of format %r on a %r engine" % (d["fmt"], self.serve))
        if lat.ndim != 2 or lat.shape != (ids.size, self.row_len):
            raise EngineError(E_INVALID, "apply_delta: rows of %r elements on an engine of row_len %d" % (lat.shape[1:], self.row_len))
        if ids.size:
            self.set_rows_raw(ids, d["lin_w"], lat)
        b = np.ascontiguousarray(d["bias"], np.float32).reshape(-1)[:1].copy()
        self._check(self.lib.ffm_engine_set_weights(self.h, _f(b), None, None))

    def load_sparse_weights(self, d):
        """sparse_state() of a training engine of the same config into this SERVING engine: the listed
        features' lin_w and vec_w (rounded to the format) and the bias; (n, z) are not looked at.  The
        engine must still hold its create-time contents -- which are the training engine's, rounded."""
        ids = np.ascontiguousarray(d["ids"], np.int32)
        if ids.size:
            self.set_rows(ids, {k: d[k] for k in ("lin_w", "vec_w") if k in d})
        b = np.ascontiguousarray(d["bias3"], np.float32)
        self._check(self.lib.ffm_engine_set_weights(self.h, _f(b[0:1].copy()), None, None))

    def get_state(self):
        if self.serve:
            raise EngineError(E_UNSUPPORTED, "a serving engine holds no accumulators: get_weights() reads what it stores")
        st = self.zero_state()
        b = np.zeros(3, np.float32)
        vw = st["vec_w"] if self.row_len else None
        vn = st["vec_n"] if self.row_len else None
        vz = st["vec_z"] if self.row_len else None
        self._check(self.lib.ffm_engine_get_weights(self.h, _f(b[0:1]), _f(st["lin_w"]), _f(vw)))
        self._check(self.lib.ffm_engine_get_state(self.h, _f(b[1:2]), _f(b[2:3]), _f(st["lin_n"]),
                                                  _f(st["lin_z"]), _f(vn), _f(vz)))
        st["bias3"] = b
        return st

    def set_state(self, st):
        st = {k: np.ascontiguousarray(v, np.float32) for k, v in st.items()}
        b = st.get("bias3")
        g = lambda k: st[k] if k in st and st[k].size else None  # noqa: E731
        self._check(self.lib.ffm_engine_set_weights(
            self.h, _f(b[0:1].copy()) if b is not None else None, _f(g("lin_w")), _f(g("vec_w"))))
        self._check(self.lib.ffm_engine_set_state(
            self.h, _f(b[1:2].copy()) if b is not None else None,
            _f(b[2:3].copy()) if b is not None else None, _f(g("lin_n")), _f(g("lin_z")),
            _f(g("vec_n")), _f(g("vec_z"))))

    ROW_KEYS = ("lin_w", "lin_n", "lin_z", "vec_w", "vec_n", "vec_z")

    def get_rows(self, ids):
        """State of the listed features only: dict of lin_* [n] and vec_* [n, row_len]."""
        ids = np.ascontiguousarray(ids, np.int32)
        n, L = ids.size, self.row_len
        keys = ("lin_w", "vec_w") if self.serve else self.ROW_KEYS  # (a serving engine: decoded w, no n / z)
        out = {k: np.zeros((n, L) if k.startswith("vec") else n, np.float32) for k in keys}
        args = [_f(out[k]) if k in out and out[k].size else None for k in self.ROW_KEYS]
        self._check(self.lib.ffm_engine_get_rows(self.h, n, _i(ids), *args))
        return out

    def set_rows(self, ids, st):
        """Overwrites the listed features' state with the given arrays (any subset of ROW_KEYS)."""
        ids = np.ascontiguousarray(ids, np.int32)
        st = {k: np.ascontiguousarray(v, np.float32) for k, v in st.items() if k in self.ROW_KEYS}
        args = [_f(st[k]) if k in st and st[k].size else None for k in self.ROW_KEYS]
        self._check(self.lib.ffm_engine_set_rows(self.h, ids.size, _i(ids), *args))

    # ---- sparse checkpoints: only what differs from a fresh engine of the same config ----
    def changed_features(self):
        """Ascending int32 ids of the features that no longer hold what the constructor gave them
        (ffm_engine_changed_features: one device scan, bit patterns compared)."""
        n = ctypes.c_int64(0)
        # ONE scan: a count-first call would scan the model twice (a fresh 33 M-feature model: every w against
        # its fp64 draw, both times).  The buffer is address space only: pages nobody writes are never committed.
        ids = np.empty(self.n_feats, np.int32)
        self._check(self.lib.ffm_engine_changed_features(self.h, _i(ids), ids.size, ctypes.byref(n)))
        return ids[:n.value].copy()

    def refresh_weights(self):
        """Sets every stored w to W(n, z) where the accumulators are live, so that prediction and
        persistence see the model that was learned (ffm_engine_refresh_weights; (n, z) untouched, the
        training trajectory unchanged).  Returns dict(lin_live, lin_nonzero, lin_moved, lat_live,
        lat_nonzero, lat_moved)."""
        st = RefreshStats()
        self._check(self.lib.ffm_engine_refresh_weights(self.h, ctypes.byref(st)))
        return st.as_dict()

    def _bias3(self):
        b = np.zeros(3, np.float32)
        self._check(self.lib.ffm_engine_get_weights(self.h, _f(b[0:1]), None, None))
        self._check(self.lib.ffm_engine_get_state(self.h, _f(b[1:2]), _f(b[2:3]), None, None, None, None))
        return b

    def sparse_state(self):
        """The model as a delta to a fresh engine of the same config: dict(ids, bias3, ROW_KEYS arrays
        of the changed features).  load_sparse_state() of it on such an engine reproduces this one bit
        for bit."""
        if self.serve:
            raise EngineError(E_UNSUPPORTED, "a serving engine holds no accumulators: the sparse checkpoint is a training engine's")
        ids = self.changed_features()
        out = dict(ids=ids, bias3=self._bias3())
        out.update(self.get_rows(ids))
        return out

    def load_sparse_state(self, d):
        """Applies sparse_state() of an engine of the same config; refused unless this engine still
        holds exactly what its constructor gave it (no changed feature)."""
        n = ctypes.c_int64(0)
        self._check(self.lib.ffm_engine_changed_features(self.h, None, 0, ctypes.byref(n)))
        if n.value != 0:
            raise EngineError(E_INVALID, "load_sparse_state needs a fresh engine: %d features already changed" % n.value)
        ids = np.ascontiguousarray(d["ids"], np.int32)
        if ids.size:
            self.set_rows(ids, d)
        b = np.ascontiguousarray(d["bias3"], np.float32)
        self._check(self.lib.ffm_engine_set_weights(self.h, _f(b[0:1]), None, None))
        self._check(self.lib.ffm_engine_set_state(self.h, _f(b[1:2]), _f(b[2:3]), None, None, None, None))

    # ---- blocks of rows in host memory ----
    def _csr(self, c):
        # numpy's .ctypes.data_as builds a fresh ctypes object per call (several microseconds each):
        # for a block that is handed over again and again (a trainer's ring of page-locked blocks)
        # the argument tuple is kept on the block, keyed by the identity of its arrays
        fld = c.field if (self.model_type == FFM or c.field is not None) else None
        key = (c.n_rows, id(c.row_ptr), id(fld), id(c.feat), id(c.val), id(c.label))
        cached = getattr(c, "_ffm_csr_args", None)
        if cached is not None and cached[0] == key:
            return cached[1]
        args = (c.n_rows, _i(c.row_ptr), _i(fld), _i(c.feat), _f(c.val), _i(c.label))
        try:
            # (the arrays ride along: while they are referenced here their ids cannot be reused)
            c._ffm_csr_args = (key, args, (c.row_ptr, fld, c.feat, c.val, c.label))
        except AttributeError:  # (a block type without a __dict__)
            pass
        return args

    def train_batch(self, c, weight=None):
        """One block with the engine's batch semantics.  Returns (logits, loss_sum).
        weight: one float32 per row (include/ffm_engine.h "Sample weights"); the loss sum is then
        sum(weight * loss).  None: the unweighted call."""
        out = np.zeros(max(c.n_rows, 1), np.float32)
        loss = ctypes.c_double(0.0)
        if weight is None:
            self._check(self.lib.ffm_engine_train_batch(self.h, *self._csr(c), _f(out),
                                                        ctypes.byref(loss)))
        else:
            _w(weight, c.n_rows)
            self._check(self.lib.ffm_engine_train_batch_weighted(self.h, *self._csr(c), _f(weight), _f(out),
                                                                 ctypes.byref(loss)))
        return out[:c.n_rows], float(loss.value)

    def train_batch_async(self, c, weight=None):
        """Pipelined: stages and groups this block, trains the one passed by the previous call."""
        if weight is None:
            self._check(self.lib.ffm_engine_train_batch_async(self.h, *self._csr(c)))
        else:
            self._check(self.lib.ffm_engine_train_batch_async_weighted(self.h, *self._csr(c), _w(weight, c.n_rows), 0))

    def train_batch_async_pinned(self, c, weight=None):
        """The same for a block in page-locked memory (pin_block): no host copy, three blocks in
        flight; the block (and its weight array, page-locked as well) stays untouched until
        blocks_pulled() has reached its ordinal."""
        if weight is None:
            self._check(self.lib.ffm_engine_train_batch_async_pinned(self.h, *self._csr(c)))
        else:
            self._check(self.lib.ffm_engine_train_batch_async_weighted(self.h, *self._csr(c), _w(weight, c.n_rows), 1))

    def stage_batch(self, c, zero_copy=False, weight=None):
        """Host block -> (pinned slot ->) HBM + grouping on the side stream (returns at once).
        zero_copy: the block's arrays are page-locked (pin_block) and stay untouched until trained."""
        if weight is None:
            self._check(self.lib.ffm_engine_stage_batch(self.h, *self._csr(c), int(zero_copy)))
        else:
            self._check(self.lib.ffm_engine_stage_batch_weighted(self.h, *self._csr(c), _w(weight, c.n_rows),
                                                                 int(zero_copy)))

    def blocks_pulled(self):
        """How many staged blocks have been uploaded so far (their host arrays may be reused)."""
        return int(self.lib.ffm_engine_blocks_pulled(self.h))

    def train_staged(self, logit_out=None, loss_sum_out=None):
        """The whole step on the oldest staged block (unsharded engines; device outputs)."""
        self._check(self.lib.ffm_engine_train_staged(self.h, logit_out, loss_sum_out))

    def pin_block(self, c):
        """Page-locks the block's five arrays in place (for stage_batch(zero_copy=True)).  Give it
        arrays that own their pages (page_aligned)."""
        for a in (c.row_ptr, c.field, c.feat, c.val, c.label):
            if a is not None and a.size:
                self._check(self.lib.ffm_engine_pin_host(a.ctypes.data, a.nbytes))

    def unpin_block(self, c):
        for a in (c.row_ptr, c.field, c.feat, c.val, c.label):
            if a is not None and a.size:
                self.lib.ffm_engine_unpin_host(a.ctypes.data)

    def train_forward_staged(self, partial_logit=None):
        """Phase 1 on the oldest staged block; follow with train_update_device."""
        self._check(self.lib.ffm_engine_train_forward_staged(self.h, partial_logit))

    def train_flush(self):
        """Trains the last staged block, waits; the loss sum of all blocks since the last flush."""
        loss = ctypes.c_double(0.0)
        self._check(self.lib.ffm_engine_train_flush(self.h, ctypes.byref(loss)))
        return float(loss.value)

    def predict_batch_async(self, c, zero_copy=False, scores=None, output_prob=False):
        """Pipelined evaluation: uploads the block on the side stream and predicts it; the loss sum
        of all blocks since the last flush comes back from train_flush().
        scores: a float32 array of at least c.n_rows elements in page-locked memory (score_buffer())
        that receives the block's logits (probabilities with output_prob), bit for bit what
        predict_batch returns; it is complete once blocks_scored() has reached the block's staging
        number, or after sync() / train_flush()."""
        if scores is None:
            self._check(self.lib.ffm_engine_predict_batch_async(self.h, *self._csr(c), int(zero_copy)))
            return
        if scores.dtype != np.float32 or scores.ndim != 1 or scores.size < c.n_rows or not scores.flags.c_contiguous:
            raise ValueError("scores: a contiguous float32 array of at least n_rows elements")
        self._check(self.lib.ffm_engine_predict_batch_async_scores(
            self.h, *self._csr(c), int(zero_copy), int(bool(output_prob)), scores.ctypes.data))

    # ---- blocks of rows that already lie in HBM (include/ffm_engine.h "Resident rows") ----
    def stage_resident(self, block):
        """stage_batch(zero_copy=True) for a RowsBlock in HBM (RowCutter.close); block.seq is its staging number."""
        self._check(self.lib.ffm_engine_stage_batch_resident(self.h, ctypes.byref(block)))

    def train_async_resident(self, block):
        """train_batch_async_pinned for a RowsBlock in HBM: three blocks in flight; the block's buffer is free
        (RowCutter.release) once blocks_pulled() has reached block.seq."""
        self._check(self.lib.ffm_engine_train_batch_async_resident(self.h, ctypes.byref(block)))

    def predict_async_resident(self, block, scores=None, output_prob=False):
        """predict_batch_async(zero_copy=True, scores=...) for a RowsBlock in HBM."""
        if scores is not None and (scores.dtype != np.float32 or scores.ndim != 1 or scores.size < block.n_rows
                                   or not scores.flags.c_contiguous):
            raise ValueError("scores: a contiguous float32 array of at least n_rows elements")
        self._check(self.lib.ffm_engine_predict_batch_async_resident(
            self.h, ctypes.byref(block), int(bool(output_prob)), None if scores is None else scores.ctypes.data))

    def blocks_scored(self):
        """Staging number of the last block whose scores are whole in its buffer (non-blocking)."""
        return int(self.lib.ffm_engine_blocks_scored(self.h))

    def score_buffer(self, n):
        """A page-locked float32 array of n elements for predict_batch_async(scores=...): pages of
        its own (page_aligned), locked in place (ffm_engine_pin_host).  Release with free_score_buffer."""
        a = page_aligned(n, np.float32)
        self._check(self.lib.ffm_engine_pin_host(a.ctypes.data, max(1, a.size) * 4))
        return a

    def free_score_buffer(self, a):
        self.lib.ffm_engine_unpin_host(a.ctypes.data)

    def train_rows(self, c):
        """Row after row (n_rows == 1 per call): the reference's sequential train() loop."""
        logits = np.zeros(c.n_rows, np.float32)
        total = 0.0
        for r in range(c.n_rows):
            lg, ls = self.train_batch(c.rows(r, r + 1))
            logits[r] = lg[0]
            total += ls
        return logits, total

    def predict_batch(self, c, output_prob=False, with_loss=True):
        out = np.zeros(max(c.n_rows, 1), np.float32)
        loss = ctypes.c_double(0.0)
        n, rp, fld, ft, v, lab = self._csr(c)
        self._check(self.lib.ffm_engine_predict_batch(self.h, n, rp, fld, ft, v,
                                                      lab if with_loss else None,
                                                      int(output_prob), _f(out),
                                                      ctypes.byref(loss)))
        return out[:c.n_rows], float(loss.value)

    def score_candidates(self, ctx, cand_req_ptr, cand, output_prob=False):
        """One context against many candidates on a serving engine (include/ffm_engine.h "Scoring
        candidates"): ctx holds one row per request, cand one row per candidate; the candidates of request r
        are rows [cand_req_ptr[r], cand_req_ptr[r + 1]) of cand.  Returns the candidates' scores: bit for bit
        predict_batch(spell_out_candidates(ctx, cand_req_ptr, cand)).  Labels are ignored; val may be None
        (every value is 1.0)."""
        rq = np.ascontiguousarray(cand_req_ptr, np.int32)
        if rq.shape != (ctx.n_rows + 1,):
            raise ValueError("cand_req_ptr needs one entry per request and one more")
        out = np.zeros(max(cand.n_rows, 1), np.float32)
        _, cp, cfld, cft, cv, _ = self._csr(ctx)
        n_cand, kp, kfld, kft, kv, _ = self._csr(cand)
        self._check(self.lib.ffm_engine_score_candidates(self.h, ctx.n_rows, cp, cfld, cft, cv, _i(rq), n_cand, kp, kfld,
                                                         kft, kv, int(output_prob), _f(out)))
        return out[:cand.n_rows]

    # ---- blocks already in HBM (raw device addresses as ints) ----
    def score_candidates_device(self, n_req, ctx_ptr, ctx_field, ctx_feat, ctx_val, cand_req_ptr, n_cand, cand_ptr,
                                cand_field, cand_feat, cand_val, ctx_nnz, cand_nnz, ctx_cap, output_prob, out):
        """score_candidates on arrays already in HBM (device addresses); ctx_cap: the longest context of the
        call.  Asynchronous on the engine's stream; sync() reports a too-long context or row."""
        self._check(self.lib.ffm_engine_score_candidates_device(
            self.h, int(n_req), ctx_ptr, ctx_field, ctx_feat, ctx_val, cand_req_ptr, int(n_cand), cand_ptr, cand_field,
            cand_feat, cand_val, int(ctx_nnz), int(cand_nnz), int(ctx_cap), int(output_prob), out))

    def train_batch_device(self, n_rows, nnz, row_ptr, field, feat, val, label, logit_out=None,
                           loss_sum_out=None, weight=None):
        """weight: device address of n_rows floats, or None."""
        if weight is None:
            self._check(self.lib.ffm_engine_train_batch_device(self.h, n_rows, nnz, row_ptr, field, feat,
                                                               val, label, logit_out, loss_sum_out))
        else:
            self._check(self.lib.ffm_engine_train_batch_device_weighted(self.h, n_rows, nnz, row_ptr, field, feat,
                                                                        val, label, weight, logit_out, loss_sum_out))

    def hash_ids_device(self, nnz, field, feat_in, feat_out):
        """The engine's id mapping (hash_ids=True engines) applied to a block already in HBM, for callers of
        the _device entry points, which take ids as they are.  Device addresses; feat_out may be feat_in;
        field None: LR / FM, or FFM rows of one entry per field in field order.  Asynchronous on the
        engine's stream."""
        self._check(self.lib.ffm_engine_hash_ids_device(self.h, int(nnz), field, feat_in, feat_out))

    def normalize_rows_device(self, n_rows, nnz, row_ptr, field, feat, val_in, val_out):
        """normalize_rows of a block already in HBM, for callers of the _device entry points, which take values as
        they are.  Device addresses; val_out may be val_in; val_in None: ones; field None: LR / FM, or FFM rows
        whose fields are all valid.  Any engine, normalize=True or not.  Asynchronous on the engine's stream."""
        self._check(self.lib.ffm_engine_normalize_rows_device(self.h, int(n_rows), int(nnz), row_ptr, field, feat, val_in, val_out))

    def norm_stats(self, reset=False):
        """(rows normalised since create or the last reset, how many of them were left as they came: zero or
        non-finite norm)."""
        rows, left = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self.lib.ffm_engine_norm_stats(self.h, 1 if reset else 0, ctypes.byref(rows), ctypes.byref(left)))
        return int(rows.value), int(left.value)

    def set_rare_fold(self, bits=None, words=None):
        """Folds rare ids in every block handed over from now on (include/ffm_engine.h "Rare ids"): words = a
        keep-map of 2^bits slots (IdCounter.keep); None turns the fold off.  hash_ids=True engines only, idle."""
        if words is None:
            self._check(self.lib.ffm_engine_set_rare_fold(self.h, 0, None))
            return
        bits, words = _rare_words(bits, words)
        self._check(self.lib.ffm_engine_set_rare_fold(self.h, bits, words.ctypes.data))

    def set_buckets(self, buckets=None):
        """Maps numeric fields to quantile buckets in every block handed over from now on (include/ffm_engine.h
        "Value buckets"): buckets = {field: edges} (bucket_edges); None takes the table off.  hash_ids=True FFM
        engines only, idle."""
        if buckets is None:
            self._check(self.lib.ffm_engine_set_buckets(self.h, None, None))
            return
        n_edges, edges = _bucket_table(self.cfg.n_fields, buckets)
        self._check(self.lib.ffm_engine_set_buckets(self.h, n_edges.ctypes.data, edges.ctypes.data))

    def bucket_ids_device(self, nnz, field, feat_in, val_in, feat_out, val_out):
        """The engine's whole mapping (bucket, fold, hash) of a block already in HBM (addresses; in place is
        fine); asynchronous on the engine's stream."""
        self._check(self.lib.ffm_engine_bucket_ids_device(self.h, int(nnz), field, feat_in, val_in, feat_out, val_out))

    def prepare_device(self, n_rows, nnz, row_ptr, field, feat, val):
        """Look-ahead: group the next block on a side stream (see include/ffm_engine.h)."""
        self._check(self.lib.ffm_engine_prepare_device(self.h, n_rows, nnz, row_ptr, field, feat, val))

    def train_forward_device(self, n_rows, nnz, row_ptr, field, feat, val, label, partial_logit, weight=None):
        """weight: device address of n_rows floats (valid until train_update_device has run), or None."""
        if weight is None:
            self._check(self.lib.ffm_engine_train_forward_device(self.h, n_rows, nnz, row_ptr, field,
                                                                 feat, val, label, partial_logit))
        else:
            self._check(self.lib.ffm_engine_train_forward_device_weighted(self.h, n_rows, nnz, row_ptr, field,
                                                                          feat, val, label, weight, partial_logit))

    def train_update_device(self, logit, logit_out=None, loss_sum_out=None):
        self._check(self.lib.ffm_engine_train_update_device(self.h, logit, logit_out, loss_sum_out))

    def predict_batch_device(self, n_rows, nnz, row_ptr, field, feat, val, label, output_prob,
                             out, loss_sum_out=None):
        self._check(self.lib.ffm_engine_predict_batch_device(self.h, n_rows, nnz, row_ptr, field,
                                                             feat, val, label, int(output_prob),
                                                             out, loss_sum_out))

    def predict_finish_device(self, n_rows, logit, label, output_prob, out, loss_sum_out=None):
        """Second phase of a sharded predict: full logits (summed across shards) -> out / loss."""
        self._check(self.lib.ffm_engine_predict_finish_device(self.h, n_rows, logit, label,
                                                              int(output_prob), out, loss_sum_out))

    def fill_state(self, seed=7, n_lo=0.05, n_hi=1.0, z_stddev=0.3):
        """Warm random accumulators drawn on the device (measurement utility)."""
        self._check(self.lib.ffm_engine_fill_state(self.h, int(seed), n_lo, n_hi, z_stddev))

    def eval_sigmoid(self, x):
        x = np.ascontiguousarray(x, np.float32)
        y = np.empty_like(x)
        self._check(self.lib.ffm_engine_eval_sigmoid(self.h, x.size, _f(x), _f(y)))
        return y

    def sync(self):
        """Waits for the stream; raises EngineError if the device flagged a block (-4: a row longer
        than max_row_nnz reached a _device entry point; that block was skipped)."""
        self._check(self.lib.ffm_engine_sync(self.h))

    check_errors = sync

    @property
    def stream(self):
        """The hipStream_t (as an int) the engine runs on."""
        return int(self.lib.ffm_engine_stream(self.h) or 0)

    # ---- AUC accumulated on the device (include/ffm_engine.h "Metrics") ----
    def metrics_enable(self, eval=False, train=False):
        """Turns the two channels on / off: eval = every labelled predict, train = the pre-update
        logits of every training block.  A channel that turns on starts from zero, one that stays
        on keeps its counts."""
        self._check(self.lib.ffm_engine_metrics_enable(self.h, (1 if eval else 0) | (2 if train else 0)))

    def metrics(self, channel, reset=False):
        """dict(n_pos, n_neg, n_nan, n_mixed_bins, auc, auc_slack) of "eval" / "train" so far.  Blocks
        that are staged and not trained yet are not in it: train_flush() first."""
        m = Metrics()
        self._check(self.lib.ffm_engine_metrics_read(self.h, _channel(channel), int(bool(reset)), ctypes.byref(m)))
        return m.as_dict()

    def metrics_histogram(self, channel):
        """(pos, neg): the channel's raw counters, two uint64 arrays of METRIC_BINS."""
        pos = np.zeros(METRIC_BINS, np.uint64)
        neg = np.zeros(METRIC_BINS, np.uint64)
        self._check(self.lib.ffm_engine_metrics_histogram(self.h, _channel(channel), pos.ctypes.data_as(_u64p),
                                                          neg.ctypes.data_as(_u64p)))
        return pos, neg

    # ---- field ablation (include/ffm_engine.h "Field ablation") ----
    def ablation_enable(self, auc=False):
        """Allocates what predict_ablated needs: (n_fields + 1) x max_batch_rows scores and losses and, with auc,
        n_fields + 1 score histograms of 16 MiB each.  FFM, one whole model on one device, n_factors in {4, 8, 16,
        32, 64}, at most 64 fields; training and serving engines."""
        self._check(self.lib.ffm_engine_ablation_enable(self.h, int(bool(auc))))

    def predict_ablated(self, c, output_prob=False, with_loss=True):
        """(out[n_fields + 1, n_rows], loss_sums[n_fields + 1]): row v is predict_batch(drop_field(c, v)) for
        v < n_fields and predict_batch(c) for v = n_fields, bit for bit, from one pass over c."""
        V = self.n_fields + 1
        out = np.zeros((V, c.n_rows), np.float32)  # (variant-major with stride n_rows: what the call writes)
        loss = np.zeros(V, np.float64)
        n, rp, fld, ft, v, lab = self._csr(c)
        self._check(self.lib.ffm_engine_predict_ablated(self.h, n, rp, fld, ft, v, lab if with_loss else None,
                                                        int(output_prob), _f(out), loss.ctypes.data_as(_f64p)))
        return out[:, :c.n_rows], loss

    def predict_ablated_device(self, n_rows, nnz, row_ptr, field, feat, val, label, output_prob, out, loss_sum_out=None):
        """predict_ablated on arrays already in HBM (device addresses; out[(n_fields + 1) * n_rows] variant-major,
        loss_sum_out[n_fields + 1]).  Asynchronous on the engine's stream; sync() reports a too-long row."""
        self._check(self.lib.ffm_engine_predict_ablated_device(self.h, int(n_rows), int(nnz), row_ptr, field, feat, val, label,
                                                               int(output_prob), out, loss_sum_out))

    def ablation_metrics(self, reset=False):
        """One dict per variant (n_fields + 1), as metrics() returns for a channel: the AUC of the model without
        field v over every labelled block predict_ablated has seen (ablation_enable(auc=True))."""
        m = (Metrics * (self.n_fields + 1))()
        self._check(self.lib.ffm_engine_ablation_read(self.h, int(bool(reset)), m))
        return [x.as_dict() for x in m]

    # ---- pair ablation (include/ffm_engine.h "Pair ablation") ----
    def pair_ablation_enable(self, auc=False):
        """Allocates what predict_pair_ablated needs: (V + 1) x max_batch_rows scores and losses, V =
        pair_count(n_fields), and, with auc, V + 1 score histograms of 16.8 MB each (13 GB at 39 fields, 35 GB at
        64).  FFM, one whole model on one device, n_factors in {4, 8, 16, 32, 64}, at most 64 fields; training
        and serving engines."""
        self._check(self.lib.ffm_engine_pair_ablation_enable(self.h, int(bool(auc))))

    def predict_pair_ablated(self, c, output_prob=False, with_loss=True, scores=True):
        """(out[V + 1, n_rows] or None, loss_sums[V + 1]): row pair_index(n_fields, f, g) is the prediction
        without the terms between fields f and g, row V is predict_batch(c), bit for bit, from one pass over c.
        scores=False leaves the scores in HBM and returns None for them: only the loss sums come back."""
        V = self.n_fields * (self.n_fields + 1) // 2 + 1
        out = np.zeros((V, c.n_rows), np.float32) if scores else None  # (variant-major with stride n_rows)
        loss = np.zeros(V, np.float64)
        n, rp, fld, ft, v, lab = self._csr(c)
        self._check(self.lib.ffm_engine_predict_pair_ablated(self.h, n, rp, fld, ft, v, lab if with_loss else None,
                                                             int(output_prob), _f(out), loss.ctypes.data_as(_f64p)))
        return out, loss

    def predict_pair_ablated_device(self, n_rows, nnz, row_ptr, field, feat, val, label, output_prob, out, loss_sum_out=None):
        """predict_pair_ablated on arrays already in HBM (device addresses; out[(V + 1) * n_rows] variant-major or
        None, loss_sum_out[V + 1]).  Asynchronous on the engine's stream; sync() reports a too-long row."""
        self._check(self.lib.ffm_engine_predict_pair_ablated_device(self.h, int(n_rows), int(nnz), row_ptr, field, feat, val,
                                                                    label, int(output_prob), out, loss_sum_out))

    def pair_ablation_metrics(self, reset=False):
        """One dict per variant (V + 1), as metrics() returns for a channel: the AUC of the model without the pair
        over every labelled block predict_pair_ablated has seen (pair_ablation_enable(auc=True))."""
        m = (Metrics * (self.n_fields * (self.n_fields + 1) // 2 + 1))()
        self._check(self.lib.ffm_engine_pair_ablation_read(self.h, int(bool(reset)), m))
        return [x.as_dict() for x in m]

    # ---- the pruning curve (include/ffm_engine.h "Pruning curve") ----
    def pair_curve_enable(self, level, cuts, auc=False):
        """Sets the level table (uint16[n_fields, n_fields], symmetric; pair_curve_levels makes a ladder's) and 1 .. 64
        cuts, each in [0, 65536], and allocates what predict_pair_curve needs: (n_cuts + 1) x max_batch_rows scores and
        losses and, with auc, n_cuts + 1 score histograms of 16.8 MB each.  Calling it again replaces table and cuts;
        with the same number of cuts the histograms keep their counts, which then mix two ladders: call
        pair_curve_metrics(reset=True) before changing the table.
        The engines of the ablations: FFM, one whole model on one device, n_factors in {4, 8, 16, 32, 64}, at most
        64 fields; training and serving engines."""
        lv = np.asarray(level)
        if lv.ndim != 2 or lv.shape[0] != lv.shape[1]:
            raise ValueError("level: a square table [n_fields, n_fields]")
        if lv.dtype.kind not in "ui" or (lv.size and (lv.min() < 0 or lv.max() > 65535)):
            raise ValueError("level: unsigned 16-bit entries")
        lv = np.ascontiguousarray(lv, np.uint16)
        ct = np.ascontiguousarray(np.asarray(cuts, np.int64).reshape(-1))
        if ct.size and (ct.min() < -(1 << 31) or ct.max() >= (1 << 31)):
            raise ValueError("a cut lies in [0, 65536]")
        ct = np.ascontiguousarray(ct, np.int32)
        self._check(self.lib.ffm_engine_pair_curve_enable(self.h, lv.ctypes.data_as(_vp), int(lv.shape[0]),
                                                          ct.ctypes.data_as(_i32p), int(ct.shape[0]), int(bool(auc))))
        self._curve_variants = int(ct.shape[0]) + 1

    def _curve_v(self):
        v = getattr(self, "_curve_variants", 0)
        if not v:
            raise EngineError(E_INVALID, "the pruning curve is off (pair_curve_enable)")
        return v

    def predict_pair_curve(self, c, output_prob=False, with_loss=True, scores=True):
        """(out[n_cuts + 1, n_rows] or None, loss_sums[n_cuts + 1]): row i is predict_batch(c) under
        set_pair_mask(pair_curve_mask(level, cuts[i])), row n_cuts is predict_batch(c), bit for bit, from one pass
        over c.  scores=False leaves the scores in HBM and returns None for them."""
        V = self._curve_v()
        out = np.zeros((V, c.n_rows), np.float32) if scores else None  # (variant-major with stride n_rows)
        loss = np.zeros(V, np.float64)
        n, rp, fld, ft, v, lab = self._csr(c)
        self._check(self.lib.ffm_engine_predict_pair_curve(self.h, n, rp, fld, ft, v, lab if with_loss else None,
                                                           int(output_prob), _f(out), loss.ctypes.data_as(_f64p)))
        return out, loss

    def predict_pair_curve_device(self, n_rows, nnz, row_ptr, field, feat, val, label, output_prob, out, loss_sum_out=None):
        """predict_pair_curve on arrays already in HBM (device addresses; out[(n_cuts + 1) * n_rows] variant-major or
        None, loss_sum_out[n_cuts + 1]).  Asynchronous on the engine's stream; sync() reports a too-long row."""
        self._check(self.lib.ffm_engine_predict_pair_curve_device(self.h, int(n_rows), int(nnz), row_ptr, field, feat, val,
                                                                  label, int(output_prob), out, loss_sum_out))

    def pair_curve_metrics(self, reset=False):
        """One dict per variant (n_cuts + 1), as metrics() returns for a channel: the AUC under each cut's mask over
        every labelled block predict_pair_curve has seen (pair_curve_enable(auc=True))."""
        m = (Metrics * self._curve_v())()
        self._check(self.lib.ffm_engine_pair_curve_read(self.h, int(bool(reset)), m))
        return [x.as_dict() for x in m]

    # ---- pair masks (include/ffm_engine.h "Pair masks") ----
    def set_pair_mask(self, keep=None):
        """Every row prediction from now on leaves out the pair terms whose fields' bit is clear.  keep: the words
        (uint64[n_fields], as pair_mask returns them) or an iterable of kept pairs (f, g); None clears the mask.
        While a mask is set, training, score_candidates and the ablation predictions are refused."""
        if keep is None:
            self._check(self.lib.ffm_engine_set_pair_mask(self.h, None, 0))
            return
        if isinstance(keep, np.ndarray) and keep.ndim == 1 and keep.dtype.kind in "ui":
            words = np.ascontiguousarray(keep, np.uint64)
        else:
            words = pair_mask(self.n_fields, keep)
        self._check(self.lib.ffm_engine_set_pair_mask(self.h, words.ctypes.data_as(_vp), int(words.shape[0])))

    def pair_mask(self):
        """The words of the mask in force (uint64[n_fields]), or None without one."""
        words = np.zeros(max(1, self.n_fields), np.uint64)
        is_set = ctypes.c_int32(0)
        self._check(self.lib.ffm_engine_get_pair_mask(self.h, words.ctypes.data_as(_vp), ctypes.byref(is_set)))
        return words[:self.n_fields] if is_set.value else None

    # ---- the grouped AUC (include/ffm_engine.h "Metrics", keyed capture) ----
    def metrics_key_field(self, field, capacity_rows=1 << 24, eval=True, train=False):
        """Keyed capture on / off: eval = every labelled block that is predicted, train = the pre-update logits of
        every training block; a row's key is its first entry of `field`, at most capacity_rows rows are kept per
        channel.  eval = train = False turns it off."""
        self._check(self.lib.ffm_engine_metrics_key_field(self.h, (1 if eval else 0) | (2 if train else 0), int(field),
                                                          int(capacity_rows)))

    def metrics_read_keyed(self, channel, reset=False):
        """dict(n_rows, n_keys, n_keys_mixed, n_rows_mixed, n_nan, n_unkeyed, n_overflow, gauc) of "eval" / "train"."""
        m = KeyedMetrics()
        self._check(self.lib.ffm_engine_metrics_read_keyed(self.h, _channel(channel), int(bool(reset)), ctypes.byref(m)))
        return m.as_dict()

    def metrics_keyed_table(self, channel):
        """dict(key, pos, neg, u2): the per-key integers of the channel's stored rows, keys ascending."""
        n = ctypes.c_int64(0)
        rc = self.lib.ffm_engine_metrics_keyed_table(self.h, _channel(channel), 0, None, None, None, None, ctypes.byref(n))
        if rc not in (0, E_CAPACITY):
            self._check(rc)
        nk = int(n.value)
        key = np.zeros(nk, np.int32)
        pos, neg, u2 = np.zeros(nk, np.int64), np.zeros(nk, np.int64), np.zeros(nk, np.uint64)
        self._check(self.lib.ffm_engine_metrics_keyed_table(self.h, _channel(channel), nk, _i(key), pos.ctypes.data_as(_i64p),
                                                            neg.ctypes.data_as(_i64p), u2.ctypes.data_as(_u64p), ctypes.byref(n)))
        return dict(key=key.astype(np.int64), pos=pos, neg=neg, u2=u2)

    # ---- kernel timing (HIP events on the engine's stream) ----
    def profile_enable(self, on=True):
        self._check(self.lib.ffm_engine_profile_enable(self.h, int(on)))

    def profile_focus(self):
        """Keep timing only the kernel that dominated so far (cheap enough for timed regions)."""
        self._check(self.lib.ffm_engine_profile_focus(self.h))

    def profile_read(self):
        n = ctypes.c_int32(0)
        ms = ctypes.c_double(0.0)
        name = ctypes.create_string_buffer(128)
        self._check(self.lib.ffm_engine_profile_read(self.h, ctypes.byref(n), ctypes.byref(ms),
                                                     name, 128))
        return name.value.decode(), int(n.value), float(ms.value)

    def profile_dump(self):
        buf = ctypes.create_string_buffer(8192)
        self._check(self.lib.ffm_engine_profile_dump(self.h, buf, 8192))
        return buf.value.decode()


class _CountingObject:
    """What FieldSketch, ValueHistogram and IdCounter share: the handle, and entries added from host or device
    arrays.  A subclass names its entry points (_prefix) and its second array (_second: name, dtype)."""
    _prefix = None
    _second = ("feat", np.int32)

    def _create(self, *args):
        self.lib = load_library()
        self.h = _vp()
        self._check(self._fn("create")(*args, ctypes.byref(self.h)))

    def _fn(self, name):
        return getattr(self.lib, self._prefix + "_" + name)

    def _check(self, rc):
        if rc != 0:
            raise EngineError(rc, self.lib.ffm_engine_last_error().decode())

    @staticmethod
    def _array(a, dtype, what):
        if a is None:
            return None
        if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.flags.c_contiguous):
            a = np.ascontiguousarray(a, dtype)
        if a.ndim != 1:
            raise ValueError("%s: a one-dimensional %s array" % (what, np.dtype(dtype).name))
        return a

    @staticmethod
    def _ids(a, what):
        return _CountingObject._array(a, np.int32, what)

    def _add(self, field, second, zero_copy):
        name, dtype = self._second
        second = self._array(second, dtype, name)
        field = self._ids(field, "field")
        if field is not None and field.size != second.size:
            raise ValueError("field and %s must be equally long" % name)
        self._check(self._fn("add")(self.h, second.size, None if field is None else field.ctypes.data,
                                    second.ctypes.data, int(bool(zero_copy))))

    def _add_device(self, nnz, field, second):
        self._check(self._fn("add_device")(self.h, int(nnz), field, second))

    def close(self):
        if self.h:
            self._fn("destroy")(self.h)
            self.h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FieldSketch(_CountingObject):
    """One HyperLogLog sketch per field, filled on the device (include/ffm_engine.h "Field sketches"): how many
    distinct ids each field of a data set holds, before a model exists.  Needs no engine."""
    _prefix = "ffm_engine_sketch"

    def __init__(self, n_fields, device=0):
        self.n_fields = int(n_fields)
        self._create(self.n_fields, int(device))

    def add(self, field, feat, zero_copy=False):
        """Counts the entries (field[p], feat[p]); field None: entry p is field p mod n_fields.  zero_copy: the
        arrays are page-locked (ffm_engine_pin_host) int32 arrays, read in place.  Back once they may be reused."""
        self._add(field, feat, zero_copy)

    def add_device(self, nnz, field, feat):
        """The same for int32 arrays in device memory (addresses; field may be None); asynchronous."""
        self._add_device(nnz, field, feat)

    def read(self):
        """(reg uint8 [n_fields, SKETCH_REGS], n_valid, n_bad) after everything added so far."""
        reg = np.zeros((self.n_fields, SKETCH_REGS), np.uint8)
        nv, nb = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self.lib.ffm_engine_sketch_read(self.h, reg.ctypes.data, ctypes.byref(nv), ctypes.byref(nb)))
        return reg, int(nv.value), int(nb.value)

    def estimate(self):
        """Distinct ids per field, float64 [n_fields]."""
        return sketch_estimate(self.read()[0])

    def set_filter(self, bits=None, words=None):
        """From now on an entry whose bit in the keep-map `words` (2^bits slots) is 0 counts as the one id RARE_ID
        of its field (include/ffm_engine.h "Rare ids"); None turns the filter off."""
        if words is None:
            self._check(self.lib.ffm_engine_sketch_set_filter(self.h, 0, None))
            return
        bits, words = _rare_words(bits, words)
        self._check(self.lib.ffm_engine_sketch_set_filter(self.h, bits, words.ctypes.data))


class ValueHistogram(_CountingObject):
    """How often every (field, bin) of numeric columns occurs, counted exactly on the device
    (include/ffm_engine.h "Value buckets").  FFM only.  Needs no engine."""
    _prefix = "ffm_engine_valhist"
    _second = ("val", np.float32)

    def __init__(self, n_fields, device=0):
        self.n_fields = int(n_fields)
        self._create(self.n_fields, int(device))

    def add(self, field, val, zero_copy=False):
        """Counts the entries (field[p], val[p]); field None: entry p is field p mod n_fields.  zero_copy:
        page-locked (ffm_engine_pin_host) int32 / float32 arrays, read in place.  Back once they may be reused."""
        self._add(field, val, zero_copy)

    def add_device(self, nnz, field, val):
        """The same for arrays in device memory (addresses; field may be None); asynchronous."""
        self._add_device(nnz, field, val)

    def read(self):
        """(counts uint64 [n_fields, BUCKET_BINS], n_valid, n_bad, n_nan) after everything added so far."""
        counts = np.zeros((self.n_fields, BUCKET_BINS), np.uint64)
        nv, nb, nn = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self.lib.ffm_engine_valhist_read(self.h, counts.ctypes.data, ctypes.byref(nv), ctypes.byref(nb),
                                                     ctypes.byref(nn)))
        return counts, int(nv.value), int(nb.value), int(nn.value)


def _text_bytes(data):
    """(address, n_bytes, keep-alive) of a text given as bytes / bytearray / memoryview / a uint8 or int8 array."""
    if isinstance(data, np.ndarray):
        if data.dtype.itemsize != 1 or not data.flags.c_contiguous or data.ndim != 1:
            raise ValueError("text: a one-dimensional contiguous array of bytes")
        return data.ctypes.data, data.size, data
    a = np.frombuffer(bytes(data) if not isinstance(data, (bytes, bytearray)) else data, np.uint8)
    return (a.ctypes.data if a.size else None), a.size, a


def parse_text_host(data, has_field=True, max_rows=None, max_nnz=None):
    """The text grammar on the host (ffm_engine_textparse_host, no device): dict(n_lines, n_rows, nnz, n_slow,
    first_slow_byte, overflow, row_ptr, field, feat, val, label) with numpy arrays cut to the block's size -- valid
    only when n_slow == 0 and overflow == 0 (else they come back empty).  Default capacities: what the bytes can hold."""
    lib = load_library()
    addr, n, keep = _text_bytes(data)
    max_rows = n // 2 + 1 if max_rows is None else int(max_rows)
    max_nnz = n // 4 + 1 if max_nnz is None else int(max_nnz)
    row_ptr = np.zeros(max_rows + 1, np.int32)
    label = np.zeros(max(max_rows, 1), np.int32)
    field, feat = np.zeros(max(max_nnz, 1), np.int32), np.zeros(max(max_nnz, 1), np.int32)
    val = np.zeros(max(max_nnz, 1), np.float32)
    blk = TextBlock()
    rc = lib.ffm_engine_textparse_host(int(bool(has_field)), addr, n, max_rows, max_nnz, _i(row_ptr), _i(field), _i(feat),
                                       _f(val), _i(label), ctypes.byref(blk))
    if rc != 0:
        raise EngineError(rc, lib.ffm_engine_last_error().decode())
    out = {k: int(getattr(blk, k)) for k in ("n_lines", "n_rows", "nnz", "n_slow", "first_slow_byte", "overflow")}
    ok = out["n_slow"] == 0 and out["overflow"] == 0
    r, e = (out["n_rows"], out["nnz"]) if ok else (0, 0)
    out.update(row_ptr=row_ptr[:r + 1] if ok else row_ptr[:0], label=label[:r], field=field[:e], feat=feat[:e], val=val[:e])
    return out


class TextParser:
    """libffm / libsvm text to a CSR block on the device (include/ffm_engine.h "Text blocks"): two slots, so that
    one chunk is copied and parsed while the caller consumes the other.  Needs no engine."""

    def __init__(self, has_field=True, max_bytes=1 << 20, max_rows=1 << 16, max_nnz=1 << 20, device=0):
        self.lib = load_library()
        self.h = _vp()
        self.max_bytes, self.max_rows, self.max_nnz = int(max_bytes), int(max_rows), int(max_nnz)
        self._keep = [None, None]
        self._check(self.lib.ffm_engine_textparse_create(int(bool(has_field)), self.max_bytes, self.max_rows, self.max_nnz,
                                                         int(device), ctypes.byref(self.h)))

    def _check(self, rc):
        if rc != 0:
            raise EngineError(rc, self.lib.ffm_engine_last_error().decode())

    def parse(self, data, slot=0, zero_copy=False):
        """Starts the parse of `data` (bytes, or an array of bytes) into `slot`; asynchronous.  zero_copy: `data` is a
        page-locked array (ffm_engine_pin_host) that stays untouched until wait(slot) returns."""
        addr, n, keep = _text_bytes(data)
        self._check(self.lib.ffm_engine_textparse_parse(self.h, int(slot), addr, n, int(bool(zero_copy))))
        self._keep[int(slot)] = keep

    def wait(self, slot=0, rows=False):
        """The block parsed into `slot`: dict(n_lines, n_rows, nnz, n_slow, first_slow_byte, overflow, row_ptr, field,
        feat, val, label) -- the arrays as device addresses, valid until the slot's next parse, and only when
        n_slow == 0 and overflow == 0.
        rows: also "row_ptr_host", the page-locked host mirror of row_ptr as an int32 array of n_rows + 1 elements (a
        view, valid until the slot's next parse; None where the arrays are not valid), and "slot" -- what
        RowCutter.take takes (include/ffm_engine.h "Resident rows")."""
        blk = TextBlock()
        if not rows:
            self._check(self.lib.ffm_engine_textparse_wait(self.h, int(slot), ctypes.byref(blk)))
            self._keep[int(slot)] = None
            return blk.as_dict()
        mirror = _vp()
        self._check(self.lib.ffm_engine_textparse_wait_rows(self.h, int(slot), ctypes.byref(blk), ctypes.byref(mirror)))
        self._keep[int(slot)] = None
        out = blk.as_dict()
        out["slot"], out["parser"], out["row_ptr_host"] = int(slot), self, None
        if mirror.value:
            out["row_ptr_host"] = np.ctypeslib.as_array(ctypes.cast(mirror.value, _i32p), shape=(int(blk.n_rows) + 1,))
        return out

    def close(self):
        if self.h:
            self.lib.ffm_engine_textparse_destroy(self.h)
            self.h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RowCutter:
    """Blocks cut out of parsed text in HBM (include/ffm_engine.h "Resident rows"): a ring of n_blocks buffers of
    max_rows rows and max_nnz entries.  take / take_host append rows to the block being assembled, close ends it
    (a RowsBlock for Engine.*_resident), release frees its buffer once the engine has pulled it, destroy frees the cutter."""

    def __init__(self, max_rows, max_nnz, n_blocks=4, device=0):
        self.lib = load_library()
        self.h = _vp()
        self.max_rows, self.max_nnz, self.n_blocks = int(max_rows), int(max_nnz), int(n_blocks)
        self._check(self.lib.ffm_engine_rowcut_create(self.max_rows, self.max_nnz, self.n_blocks, int(device), ctypes.byref(self.h)))

    def _check(self, rc):
        if rc != 0:
            raise EngineError(rc, self.lib.ffm_engine_last_error().decode())

    def take(self, src, r0, r1):
        """Rows [r0, r1) of `src`, what TextParser.wait(slot, rows=True) returned; asynchronous."""
        self._check(self.lib.ffm_engine_rowcut_take(self.h, src["parser"].h, int(src["slot"]), int(r0), int(r1)))

    def take_host(self, n_rows, row_ptr, field, feat, val, label):
        """n_rows rows the host parsed: row_ptr [n_rows + 1] may start anywhere, field / feat / val begin at entry
        row_ptr[0] and label at the first row (int32 / float32 arrays)."""
        for a, t in ((row_ptr, np.int32), (field, np.int32), (feat, np.int32), (val, np.float32), (label, np.int32)):
            if a is not None and (a.dtype != t or not a.flags.c_contiguous):
                raise ValueError("take_host: contiguous int32 / float32 arrays")
        self._check(self.lib.ffm_engine_rowcut_take_host(self.h, int(n_rows), _i(row_ptr), _i(field), _i(feat), _f(val), _i(label)))

    def close(self):
        """Ends the block being assembled: its RowsBlock.  (The cutter itself goes with destroy().)"""
        blk = RowsBlock()
        self._check(self.lib.ffm_engine_rowcut_close(self.h, ctypes.byref(blk)))
        return blk

    def release(self, block):
        """The block's buffer may be written again (the engine has pulled it: blocks_pulled() >= block.seq)."""
        self._check(self.lib.ffm_engine_rowcut_release(self.h, int(block.index if isinstance(block, RowsBlock) else block)))

    def destroy(self):
        if self.h:
            self.lib.ffm_engine_rowcut_destroy(self.h)
            self.h = _vp()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class IdCounter(_CountingObject):
    """How often every hashed slot occurs, counted on the device up to a cap (include/ffm_engine.h "Rare ids"),
    and the keep-map of a minimum count.  n_fields 0: LR / FM.  Needs no engine."""
    _prefix = "ffm_engine_idcount"

    def __init__(self, n_fields, bits, cap, device=0):
        self.n_fields, self.bits, self.cap = int(n_fields), int(bits), int(cap)
        self._create(self.n_fields, self.bits, self.cap, int(device))

    def add(self, field, feat, zero_copy=False):
        """Counts the entries (field[p], feat[p]); field None: LR / FM, or entry p is field p mod n_fields.
        zero_copy: page-locked (ffm_engine_pin_host) int32 arrays, read in place.  Back once they may be reused."""
        self._add(field, feat, zero_copy)

    def add_device(self, nnz, field, feat):
        """The same for int32 arrays in device memory (addresses; field may be None); asynchronous."""
        self._add_device(nnz, field, feat)

    def read(self):
        """(counts uint32 [2^bits] = min(count, cap), n_valid, n_bad) after everything added so far."""
        counts = np.zeros(1 << self.bits, np.uint32)
        nv, nb = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self.lib.ffm_engine_idcount_read(self.h, counts.ctypes.data, ctypes.byref(nv), ctypes.byref(nb)))
        return counts, int(nv.value), int(nb.value)

    def keep(self, min_count):
        """(words uint64 [2^bits / 64], n_kept_slots, n_folded_entries): bit j of word i is set iff slot 64 i + j
        was counted at least min_count times; 1 <= min_count <= cap."""
        words = np.zeros((1 << self.bits) // 64, np.uint64)
        nk, nf = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self.lib.ffm_engine_idcount_keep(self.h, int(min_count), words.ctypes.data, ctypes.byref(nk),
                                                     ctypes.byref(nf)))
        return words, int(nk.value), int(nf.value)


class Group:
    """Several field-pair shard engines in ONE process (ffm_group_*): one engine per entry of
    `devices`, one RCCL all-reduce of the partial logits per block when the devices are distinct
    (a kernel sum when they share a device: one-GPU dry run of the orchestration)."""

    def __init__(self, devices, model_type="FFM", n_feats=10000, n_fields=8, n_factors=16, w_alpha=1e-4,
                 w_beta=1.0, w_l1=0.1, w_l2=5.0, init_mean=0.0, init_stddev=0.02, seed=42,
                 max_batch_rows=8192, max_batch_nnz=None, skip_init=False, max_row_nnz=0,
                 field_start=None, learn=False, hash_ids=False, normalize=False):
        """normalize: refused by the library (a shard does not own whole rows); here so that the refusal is the engine's."""
        self.lib = load_library()
        cfg = Config()
        self.lib.ffm_engine_default_config(ctypes.byref(cfg))
        cfg.model_type = MODEL_TYPES[model_type] if isinstance(model_type, str) else int(model_type)
        cfg.n_feats, cfg.n_fields, cfg.n_factors = int(n_feats), int(n_fields), int(n_factors)
        cfg.w_alpha, cfg.w_beta, cfg.w_l1, cfg.w_l2 = w_alpha, w_beta, w_l1, w_l2
        cfg.init_mean, cfg.init_stddev, cfg.seed = init_mean, init_stddev, int(seed)
        cfg.max_batch_rows = int(max_batch_rows)
        cfg.max_batch_nnz = int(max_batch_nnz if max_batch_nnz else max_batch_rows * 64)
        cfg.flags = ((FLAG_SKIP_INIT if skip_init else 0) | (FLAG_LEARN if learn else 0) | (FLAG_HASH_IDS if hash_ids else 0)
                     | (FLAG_NORM_ROWS if normalize else 0))
        cfg.max_row_nnz = int(max_row_nnz)
        self._field_start = None
        if field_start is not None:
            self._field_start = np.ascontiguousarray(field_start, np.int32)
            cfg.field_start = _i(self._field_start)
        dev = np.ascontiguousarray(devices, np.int32)
        self.h = _vp()
        rc = self.lib.ffm_group_create(ctypes.byref(cfg), dev.size, _i(dev), ctypes.byref(self.h))
        if rc != 0:
            raise EngineError(rc, self.lib.ffm_engine_last_error().decode())
        self.size = int(self.lib.ffm_group_size(self.h))
        self.collective = self.lib.ffm_group_collective(self.h).decode()
        # borrowed handles to the shards (for set_state / get_state in tests); the group owns them
        self.engines = []
        for r in range(self.size):
            e = Engine.__new__(Engine)
            e.lib, e.cfg, e.model_type, e.serve = self.lib, cfg, cfg.model_type, None
            e.h = _vp(self.lib.ffm_group_engine(self.h, r))
            e._field_start = self._field_start
            e.n_feats, e.n_fields, e.n_factors = cfg.n_feats, cfg.n_fields, cfg.n_factors
            e.row_len = int(self.lib.ffm_engine_row_len(e.h))
            e.close = lambda: None  # noqa: E731  (never destroys: the group does)
            self.engines.append(e)

    def _check(self, rc):
        if rc != 0:
            raise EngineError(rc, self.lib.ffm_engine_last_error().decode())

    def _csr(self, c):
        return self.engines[0]._csr(c)

    def train_batch(self, c, weight=None):
        out = np.zeros(max(c.n_rows, 1), np.float32)
        loss = ctypes.c_double(0.0)
        if weight is None:
            self._check(self.lib.ffm_group_train_batch(self.h, *self._csr(c), _f(out), ctypes.byref(loss)))
        else:
            _w(weight, c.n_rows)
            self._check(self.lib.ffm_group_train_batch_weighted(self.h, *self._csr(c), _f(weight), _f(out),
                                                                ctypes.byref(loss)))
        return out[:c.n_rows], float(loss.value)

    def train_batch_async(self, c, zero_copy=False, weight=None):
        if weight is None:
            self._check(self.lib.ffm_group_train_batch_async(self.h, *self._csr(c), int(zero_copy)))
        else:
            self._check(self.lib.ffm_group_train_batch_async_weighted(self.h, *self._csr(c), _w(weight, c.n_rows),
                                                                      int(zero_copy)))

    def train_flush(self):
        loss = ctypes.c_double(0.0)
        self._check(self.lib.ffm_group_train_flush(self.h, ctypes.byref(loss)))
        return float(loss.value)

    def blocks_pulled(self):
        return int(self.lib.ffm_group_blocks_pulled(self.h))

    def predict_batch(self, c, output_prob=False, with_loss=True):
        out = np.zeros(max(c.n_rows, 1), np.float32)
        loss = ctypes.c_double(0.0)
        n, rp, fld, ft, v, lab = self._csr(c)
        self._check(self.lib.ffm_group_predict_batch(self.h, n, rp, fld, ft, v, lab if with_loss else None,
                                                     int(output_prob), _f(out), ctypes.byref(loss)))
        return out[:c.n_rows], float(loss.value)

    def metrics_enable(self, eval=False, train=False):
        """Engine.metrics_enable on the rank that keeps the channels (rank 0)."""
        self._check(self.lib.ffm_group_metrics_enable(self.h, (1 if eval else 0) | (2 if train else 0)))

    def metrics(self, channel, reset=False):
        m = Metrics()
        self._check(self.lib.ffm_group_metrics_read(self.h, _channel(channel), int(bool(reset)), ctypes.byref(m)))
        return m.as_dict()

    def metrics_histogram(self, channel):
        return self.engines[0].metrics_histogram(channel)

    def refresh_weights(self):
        """Engine.refresh_weights on every shard (ffm_group_refresh_weights); the counters summed."""
        st = RefreshStats()
        self._check(self.lib.ffm_group_refresh_weights(self.h, ctypes.byref(st)))
        return st.as_dict()

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.ffm_group_destroy(self.h)
            self.h = _vp()
            self.engines = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
