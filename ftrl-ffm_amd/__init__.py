"""MI355X-native FTRL LR/FM/FFM trainer: hand-written HIP kernels for gfx950 behind the C ABI of
include/ffm_engine.h (csrc/), plus the host-side mirror of the reference's model/trainer interface
(host/) and this thin ctypes binding (engine.py).  No CPU fallback: importing is cheap, but
creating an Engine without libffm_engine.so or without a GPU raises."""
from . import build as _build
from .engine import (ABI, FFM, FM, LR, METRIC_BINS, METRIC_EVAL, METRIC_TRAIN, Config, Engine,  # noqa: F401
                     EngineError, FieldSketch, Group, KeyedMetrics, LIB_PATH, Metrics, default_batch_ramp, hash_ids, init_weights_host,
                     keyed_auc_reference, metrics_from_keyed,
                     load_library, metrics_from_histogram, page_aligned, shard_plan, sketch_estimate, field_ranges, spell_out_candidates, drop_field,
                     pair_count, pair_index, pair_fields, drop_pair_weights, pair_mask, pair_mask_pairs, pair_mask_top, pair_curve_levels, pair_curve_mask,
                     IdCounter, RARE_ID, fold_rare, rare_slot,
                     ValueHistogram, BUCKET_BINS, BUCKET_MAX_EDGES, BUCKET_NAN_ID, value_bins, bucket_edges, bucket_ids,
                     FLAG_NORM_ROWS, normalize_rows, normalize_rows_host,
                     TextParser, TextBlock, parse_text_host, TEXT_MAX_LINE, TEXT_TILE_BYTES, TEXT_SCAN_BYTES, TEXT_LINE_TILE,
                     TEXT_SCAN_CHUNK, RowCutter, RowsBlock)


def build(force=False, verbose=False):
    """Compile libffm_engine.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    return _build.build(force=force, verbose=verbose)


def build_host(force=False, verbose=False):
    """Compile the C++ host mirror (host/): the trainer CLI and its test executable."""
    return _build.build_host(force=force, verbose=verbose)
