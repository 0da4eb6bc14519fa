// cmd_option.h -- flags of the trainer.  Names and defaults are the reference's
// (src/include/utils/cmd_option.h:29-66, src/utils/cmd_option.cpp:61-114); the last block is new.
#pragma once
#include <cstdint>
#include <string>
#include <string_view>
#include <vector>

struct config_options {
  std::string model_path, train_path, eval_path;
  std::string model_type = "FFM";
  std::string file_type;
  float init_mean = 0.0f, init_stddev = 0.02f;
  float w_alpha = 1e-4f, w_beta = 1.0f, w_l1 = 0.1f, w_l2 = 5.0f;
  int thread_num = 1;  // host threads for parsing; the model update itself runs on the GPU
  int epoch = 1;
  int n_fields = 8, n_feats = 10000, n_factors = 16;
  bool cmd = false;
  bool online = true;
  // --- new: the mini-batch scheduler that replaces the per-sample thread pool ---
  int batch_size = 4096;   // --batch_size: rows per block handed to the engine
  int batch_ramp = -1;     // --batch_ramp: block size <= rows_seen / ramp (0 = off; -1 = the engine's default
                           //   for w_alpha, ffm_engine_default_batch_ramp: 32 at the reference's rates); DESIGN.md
  uint64_t seed = 42;      // --seed: weight init and the offline shuffle (the reference is unseeded)
  int device = 0;          // --device: HIP device ordinal
  bool learn = false;      // --learn: FFM_FLAG_LEARN, the opt-in variant in which the factors train
  int n_gpus = 1;          // --n_gpus: field-pair shards, one engine per device, RCCL all-reduce per block
  std::string field_ranges = "none";  // --field_ranges uniform: field f owns ids [f*n_feats/F, (f+1)*n_feats/F)
                                      //   (the layout of python/generate_data.py:272-306): shards then store
                                      //   only their slots; none: every shard keeps whole records
  // --field_ranges counted: the ranges are sized by the fields' cardinalities, counted on the device in one pass
  // over --train_data before a model exists; @PATH: read from a file of n_fields + 1 integers, one per line
  // (field_ranges.h).  field_start: what either resolved to (filled by main.cpp before a model exists; empty:
  // uniform or none, as ever).  --field_ranges_out PATH writes the ranges in that format.
  std::vector<int32_t> field_start;
  std::string field_ranges_out;
  std::string checkpoint_path;  // --checkpoint_path: write a sparse resumable checkpoint after training
  std::string resume_from;      // --resume_from: load one before training; --n_epochs then counts MORE epochs
  std::string metrics = "none";  // --metrics auc: one AUC line after every loss line (accumulated on the device)
  std::string predict_path, predict_out;  // --predict_data / --predict_out: score a file after training, one line per row
  bool predict_prob = true;               // --predict_output prob | logit
  // --pos_weight / --neg_weight / --weight_data: per-row training weights (sample_weights.h)
  float pos_weight = 1.0f, neg_weight = 1.0f;
  std::string weight_path;
  bool weights_given = false;  // one of the three was passed: training blocks carry a weight array
  bool refresh_weights = false;  // --refresh_weights: every stored w = W(n, z) before it is evaluated, saved or scored
  bool hash_feats = false;  // --hash_feats: FFM_FLAG_HASH_IDS, ids hashed into their field's id range on the device
  // --normalize_rows: FFM_FLAG_NORM_ROWS, every row scaled to unit Euclidean length on the device (include/ffm_engine.h
  // "Normalised rows"); every engine of the run that takes rows, one GPU
  bool normalize_rows = false;
  // --device_parse: the counting pre-passes (--bucket_fields, --min_count, --field_ranges counted) read --train_data
  // as raw bytes and parse them on the device (include/ffm_engine.h "Text blocks", text_stream.h); no result changes
  bool device_parse = false;
  // --device_rows: online training, evaluation and --predict_data read their files as raw bytes, the device parses
  // them and cuts the blocks in HBM (include/ffm_engine.h "Resident rows", row_stream.h); no result changes
  bool device_rows = false;
  // --serve_weights none | f32 | f16: score a saved model from a serving engine (FFM_FLAG_SERVE_F32 / _F16: the
  // weights alone, in fp32 bits or IEEE binary16); only with --resume_from ck --n_epochs 0
  std::string serve_weights = "none";
  // --compact_rows: blocks whose values are all 1.0f / whose rows are one entry per field in field order cross
  // PCIe without their val / field array (include/ffm_engine.h "Rows without values"); no result changes by a bit
  bool compact_rows = false;
  // --auc_key_field F / --auc_key_rows N: after every AUC line one more with the grouped AUC, the AUC inside each
  // value of field F averaged by impressions (include/ffm_engine.h "Metrics", keyed capture); -1 = not asked for
  int auc_key_field = -1;
  long long auc_key_rows = 16777216;
  // --field_importance true: after the last evaluation, the eval loss (and, with --metrics auc, the AUC) of the model
  // without each field, from one more pass over --eval_data (include/ffm_engine.h "Field ablation", importance.h)
  bool field_importance = false;
  // --pair_importance true: the same for every field pair -- the model without the interaction of fields f and g,
  // all n_fields (n_fields + 1) / 2 of them from one more pass (include/ffm_engine.h "Pair ablation", importance.h)
  bool pair_importance = false;
  // --pair_keep N --pair_mask_out FILE (with --pair_importance true): the N pairs whose removal costs most, written as a
  // mask file (pair_mask.h); -1 = not asked for.  --pair_mask @FILE (a run that trains nothing): the loaded model
  // predicts with the file's pairs only (include/ffm_engine.h "Pair masks")
  int pair_keep = -1;
  std::string pair_mask_out, pair_mask;
  // --pair_curve LIST|auto (with --pair_importance true): after the pairs' pass, one more pass over --eval_data gives the
  // loss (and AUC) of "keep the best N pairs" for every listed N at once (include/ffm_engine.h "Pruning curve").
  // pair_curve is the flag as given ("" = not asked for); pair_curve_keep its N, ascending and without duplicates
  // (auto: round(i V / 63), i = 0 .. 63), made once --n_fields is known.  --pair_loss_budget T (with --pair_curve and
  // --pair_mask_out, in place of --pair_keep): the mask of the smallest listed N whose per-row loss delta is <= T.
  std::string pair_curve;
  std::vector<int> pair_curve_keep;
  bool pair_loss_budget_set = false;
  double pair_loss_budget = 0.0;
  // --publish_path PREFIX [--publish_weights f32|f16]: after every epoch's training (and refresh) a serving delta
  // PREFIX.<epochs_done>.delta -- what a shadow serving engine had to move to follow the model (serve_delta.h)
  std::string publish_path, publish_weights = "f32";
  // --apply_deltas PREFIX[:N] with --serve_weights fmt --n_epochs 0: a fresh serving engine brought to the published
  // model by PREFIX.1.delta .. (apply_deltas_n = 0: every consecutive file that exists)
  std::string apply_deltas;
  int apply_deltas_n = 0;
  // --min_count T: ids seen fewer than T times in --train_data share one id per field (include/ffm_engine.h "Rare
  // ids"): counted on the device in one pass before a model exists; 0 and 1 both mean off.  --rare_bits B: the
  // counter has 2^B slots (0 = the smallest B with 2^B >= 4 * n_feats, inside [16, 30]).  --rare_ids @FILE: the
  // keep-map of an earlier run (rare_ids.h); --rare_ids_out FILE writes it.  rare_map_bits / rare_words: what either
  // resolved to (filled by main.cpp before a model exists; empty: no fold).
  int min_count = 0, rare_bits = 0;
  std::string rare_ids, rare_ids_out;
  int rare_map_bits = 0;
  std::vector<uint64_t> rare_words;

  // --bucket_fields LIST (such as 0-12,20) with --n_buckets B: the numeric fields whose values become quantile buckets
  // (include/ffm_engine.h "Value buckets"), their histograms counted on the device in one pass over --train_data before
  // a model exists.  --buckets @FILE: the table of an earlier run (value_buckets.h); --buckets_out FILE writes it.
  // bucket_field_list: the parsed LIST, ascending, no repeats.  bucket_n_edges / bucket_edges: what either resolved to,
  // as ffm_engine_set_buckets takes it (filled by main.cpp before a model exists; empty: no table).
  std::string bucket_fields, buckets, buckets_out;
  int n_buckets = 32;
  std::vector<int> bucket_field_list;
  std::vector<int32_t> bucket_n_edges;
  std::vector<uint16_t> bucket_edges;

  void parse_option(int argc, char *argv[]);  // throws std::invalid_argument like the reference
};

std::string detect_file_type(const std::string &file_path);  // cmd_option.cpp:35-59
extern const std::string_view cmd_help;
