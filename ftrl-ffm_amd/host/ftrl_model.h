// ftrl_model.h -- host-side mirror of the reference's model interface
// (src/include/model/ftrl_model.h:14-51, ffm.h:11-33, fm.h:11-28, lr.h:10-17) over the C ABI of
// include/ffm_engine.h.  Same class names, same train()/predict() meaning and return values, same
// public members; the arithmetic happens in HBM behind an ffm_engine handle.
//
//   float train(feat_vec&, int)   one reference train(): returns the pre-update logit and erases
//                                 out-of-range entries from the caller's vector, as the reference.
//   float predict(feat_vec&, bool)
//   train_block / predict_block   the same for a block of rows (what the trainers call).
//
// bias / lin_w / vec_w are host mirrors of the device weights, as public as in the reference
// (ftrl_model.h:35-37, ffm.h:25, fm.h:20).  bias and lin_w (4 bytes per feature) are pulled at
// construction; vec_w is LAZY: `model.vec_w.size()` and `model.vec_w[i].size()` answer without
// moving anything, `model.vec_w[i]` pulls row i from HBM the first time it is touched, whole-model
// walks (begin()/end(), pull_all()) pull everything -- the 33 M-feature headline model has 82 GB of
// vec_w, which no constructor should copy.  pull_weights() refreshes what is mirrored after
// training, push_weights() writes edited mirrors back (the reference's tests poke them directly).
// Model files are streamed record chunk by record chunk (persist.h): host memory stays bounded.
#pragma once
#include <algorithm>
#include <memory>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "../../include/ffm_engine.h"
#include "cmd_option.h"
#include "types.h"

namespace ftrl {

class FtrlModel;

// std::vector<std::vector<float>>-shaped view of the latent weights in HBM (see the file comment).
class LatentMirror {
 public:
  using row = std::vector<float>;
  size_t size() const { return n_; }
  bool empty() const { return n_ == 0; }
  row &operator[](size_t i);
  row &at(size_t i);
  std::vector<row>::iterator begin() { pull_all(); return dense_.begin(); }
  std::vector<row>::iterator end() { pull_all(); return dense_.end(); }
  // `a.vec_w = b.vec_w` copies the VALUES of b's rows (all of them: b is pulled) into a's mirror;
  // a.push_weights() then writes them to a's device
  LatentMirror() = default;
  LatentMirror(const LatentMirror &) = delete;
  LatentMirror &operator=(const LatentMirror &o) {
    if (this != &o) {
      const_cast<LatentMirror &>(o).pull_all();
      dense_ = o.dense_;
      dense_ready_ = true;
      cache_.clear();
    }
    return *this;
  }
  void pull_all();                    // every row, dense (small models, the reference's tests)
  bool is_dense() const { return dense_ready_; }
  size_t rows_mirrored() const { return dense_ready_ ? n_ : cache_.size(); }

 private:
  friend class FtrlModel;
  FtrlModel *owner_ = nullptr;
  size_t n_ = 0, row_len_ = 0;
  bool dense_ready_ = false;
  std::vector<row> dense_;
  std::unordered_map<size_t, row> cache_;  // rows touched one by one
};

// what a trainer saves with a checkpoint and continues from (trainer.h)
struct TrainProgress {
  long long rows_seen = 0, epochs_done = 0;
};

class FtrlModel {
 public:
  explicit FtrlModel(const config_options &opt, int model_type);
  virtual ~FtrlModel();
  FtrlModel(const FtrlModel &) = delete;
  FtrlModel &operator=(const FtrlModel &) = delete;

  virtual float train(feat_vec &features, int label);
  virtual float predict(feat_vec &features, bool output_prob);
  virtual void remove_out_range(feat_vec &feats);

  // Block entry points used by FtrlOffline / FtrlOnline.  Return sum of loss(y, logit).
  // A training block whose `weight` array is not empty (one float per row; include/ffm_engine.h "Sample
  // weights") goes through the *_weighted entry points: its gradients are scaled row by row and the
  // sums returned are sum(weight * loss).  Where a block is split into several calls, so are its weights.
  double train_block(const CsrBlock &blk, float *logit_out = nullptr);
  double predict_block(const CsrBlock &blk, bool output_prob, float *out = nullptr);
  // Pipelined training for callers that need only the loss (the trainers): queue blocks, then
  // train_flush() returns the sum of loss(y, logit) over all blocks queued since the last flush.
  // The block's arrays may be reused as soon as train_block_async returns.
  void train_block_async(const CsrBlock &blk);
  double train_flush();
  // The same without the host copy, for blocks gathered in page-locked memory: pin_block() sizes a
  // block's arrays for one engine call and page-locks them (false: could not, use the copying
  // path); train_block_pinned() hands such a block over -- it must then stay untouched until
  // blocks_pulled() has reached the number it returns (blocks handed over so far).  A block that
  // does not fit one engine call goes through the copying path instead.
  // with_weights: the block's weight array is sized and page-locked too (a ring of weighted blocks)
  bool pin_block(CsrBlock &blk, bool with_weights = false);
  void unpin_block(CsrBlock &blk);
  long long train_block_pinned(const CsrBlock &blk);
  long long blocks_pulled();
  // Pipelined evaluation (Evaluator::run_task, evaluate.cpp:23-33, needs the loss only): the block
  // is uploaded on the side stream while the previous one is predicted; `pinned`: a pin_block()ed
  // block, pulled in place and untouched until blocks_pulled() has reached the returned ordinal.
  // eval_flush() waits and returns the sum of loss(y, predict(x)) since the last flush.
  // With `scores` the block's predictions come back as well, one float per row (logits, or
  // probabilities with output_prob), the bits predict_block(blk, output_prob, out) gives.  When
  // `scores` lies in memory page-locked by pin_scores() and the block fits one engine call, they are
  // written by the device behind the block's predict kernel (ffm_engine_predict_batch_async_scores):
  // *complete = false, and they are whole once blocks_scored() has reached the returned ordinal, or
  // after eval_flush().  Otherwise -- a group (--n_gpus > 1: the synchronous ffm_group_predict_batch is
  // the only way there), a block split into several calls, a buffer that is not page-locked -- they
  // are written before the call returns: *complete = true.
  long long predict_block_async(const CsrBlock &blk, bool pinned, float *scores = nullptr, bool output_prob = false,
                                bool *complete = nullptr);
  double eval_flush();
  // --device_rows: the same three for a block that already lies in HBM (include/ffm_engine.h "Resident rows"; a closed
  // block of a row cutter, row_stream.h): ffm_engine_stage_batch_resident, _train_batch_async_resident (three blocks in
  // flight, as train_block_pinned) and _predict_batch_async_resident (scores: page-locked by pin_scores, or null).
  // The block's buffer is free once blocks_pulled() has reached the ordinal returned (also left in blk.seq).  One
  // engine only; a row beyond the engine's row capacity throws the std::length_error of the host forms.
  long long stage_block_resident(ffm_rows_block &blk);
  long long train_block_resident(ffm_rows_block &blk);
  long long predict_block_resident(ffm_rows_block &blk, float *scores = nullptr, bool output_prob = false);
  // what one engine call takes: the rows and entries of a block
  size_t block_rows_capacity() const { return static_cast<size_t>(max_rows_); }
  size_t block_nnz_capacity() const { return static_cast<size_t>(max_nnz_); }
  // Ordinal of the last block whose scores are whole (non-blocking, never decreases; may be asked
  // from another thread than the one that hands blocks over); 0 for a group.
  long long blocks_scored();
  // Page-locks [p, p + n) for predict_block_async's scores; give it pages of its own (PageAllocator).
  // false: no page-locked memory to be had (the scores then come back synchronously).
  bool pin_scores(float *p, size_t n);
  void unpin_scores(float *p);
  int n_gpus() const { return n_gpus_; }
  // --compact_rows: prints `compact rows: V of B blocks without values, F without fields` -- of the B engine
  // calls the block entry points made, how many passed val == NULL / field == NULL (nothing without the flag)
  void print_compact_rows() const;
  // --normalize_rows: `normalized rows: R scaled, U left as they came (zero or non-finite norm)`, the engine's counts
  // of every row it took so far (training and evaluation); nothing without the flag
  void print_norm_rows();
  // AUC accumulated on the device (include/ffm_engine.h "Metrics"), one engine or a group alike:
  // `eval` takes every labelled predict, `train` the pre-update logits of every training block.
  // read_metrics(FFM_METRIC_EVAL / FFM_METRIC_TRAIN) returns the channel's numbers so far (after a
  // train_flush() / eval_flush(): everything handed over) and, with reset, starts it from zero.
  void enable_metrics(bool eval, bool train);
  ffm_metrics read_metrics(int channel, bool reset);
  bool metrics_on(int channel) const { return (metrics_mask_ >> channel) & 1; }
  // The grouped AUC (include/ffm_engine.h "Metrics", keyed capture): the rows of the same two channels kept with
  // their key, the first entry of `field`; at most capacity_rows per channel.  A model made from options with
  // --auc_key_field turns it on and off together with enable_metrics.  One FFM engine only (throws otherwise).
  void enable_keyed_metrics(int field, long long capacity_rows, bool eval, bool train);
  ffm_keyed_metrics read_keyed_metrics(int channel, bool reset);
  bool keyed_metrics_on(int channel) const { return (keyed_mask_ >> channel) & 1; }
  // Every stored w from its accumulators (include/ffm_engine.h "Refresh"), one engine or a group alike:
  // what prediction and the model files read is otherwise one update behind (n, z).  Blocks queued and
  // not trained yet are trained first (their losses stay in train_flush()'s sum).  The host mirrors
  // (bias, lin_w, vec_w) are pulled again / dropped, as after load_checkpoint.  Returns the six counts.
  ffm_refresh_stats refresh_weights();
  // Ablation (include/ffm_engine.h "Field ablation", "Pair ablation"): the loss -- and, with_auc, the AUC -- of this
  // model without each field (Fields: n_fields + 1 variants) or without the interaction of fields f and g (Pairs:
  // ffm_engine_pair_count(n_fields) + 1 variants), all from one pass; the last variant is the rows themselves.
  // ablation_variants is that count (throws for the pairs of more than 64 fields).  enable_ablation allocates the
  // engine's scratch (one FFM engine only: throws otherwise); predict_ablated_block runs one block through the
  // synchronous call and ADDS its per-variant loss sums to loss_sums[variants] (the scores stay on the device);
  // read_ablation_metrics returns the variants' numbers so far and, with reset, starts them from zero.
  enum class Ablation { Fields, Pairs };
  size_t ablation_variants(Ablation kind) const;
  void enable_ablation(Ablation kind, bool with_auc);
  void predict_ablated_block(Ablation kind, const CsrBlock &blk, std::vector<double> &loss_sums);
  std::vector<ffm_metrics> read_ablation_metrics(Ablation kind, bool reset);
  // Pruning curve (include/ffm_engine.h "Pruning curve"; pair_mask.h makes the table): level[n_fields * n_fields] and 1 ..
  // 64 cuts give cuts.size() + 1 variants, the rows themselves last.  enable_pair_curve sets them on the one FFM engine
  // (throws std::invalid_argument with the engine's reason when it refuses); predict_curve_block ADDS one block's
  // per-variant loss sums to loss_sums[cuts.size() + 1]; read_curve_metrics as read_ablation_metrics.
  void enable_pair_curve(const std::vector<uint16_t> &level, const std::vector<int32_t> &cuts, bool with_auc);
  void predict_curve_block(const CsrBlock &blk, std::vector<double> &loss_sums);
  std::vector<ffm_metrics> read_curve_metrics(bool reset);
  // Pair mask (include/ffm_engine.h "Pair masks"; pair_mask.h makes the words): from now on every prediction of this
  // model leaves out the terms of the pairs whose bit is clear, and training is refused.  keep[n_fields]; one FFM
  // engine only (throws std::invalid_argument otherwise, with the engine's reason).
  void set_pair_mask(const std::vector<uint64_t> &keep);

  // Model files in the reference's formats (ffm.cpp:138-200, lr.cpp:26-39); available for every
  // model type here (the reference has none for FM).  save_state/load_state add the FTRL
  // accumulators, which make a checkpoint resumable.
  void save_model(std::string_view file_name);
  void load_model(std::string_view file_name);
  void save_compressed_model(std::string_view file_name, int compress_level);
  void load_compressed_model(std::string_view file_name);
  void save_state(std::string_view file_name, int compress_level = 3);
  void load_state(std::string_view file_name);
  // Sparse resumable checkpoint (persist.h): only the features that no longer hold what the
  // constructor gave them (ffm_engine_changed_features, one device scan), their full records
  // (w, n, z), the bias triple and the trainer's progress.  load_checkpoint wants a model built with the
  // same shape, seed, init parameters, --learn and --hash_feats setting that has not been touched yet (throws std::runtime_error
  // otherwise) and makes it the saved model bit for bit; returns the progress saved with it.  Not
  // supported for sharded models (--n_gpus > 1): both throw.
  using TrainProgress = ftrl::TrainProgress;
  void save_checkpoint(std::string_view file_name, int compress_level = 3, TrainProgress progress = TrainProgress());
  TrainProgress load_checkpoint(std::string_view file_name);

  // Serving deltas (serve_delta.h; include/ffm_engine.h "Serving deltas").
  // publish_delta, on a training model (one FFM engine): a SHADOW serving engine of format `fmt` ("f32" / "f16")
  // on the same device, made by the first call (or by prepare_publish), is synced from the training engine; the
  // ids it had to move and their raw rows, pulled chunk by chunk, go to PREFIX.<seq>.delta.  The shadow costs a
  // third (f32) or a sixth (f16) of the training engine's memory on top of it.
  // prepare_publish makes the shadow and brings it to a resumed run's epoch by applying PREFIX.1 .. PREFIX.<seq_done>
  // (throws std::runtime_error on a missing or mismatching file).
  // apply_delta, on a serving model: checks every header field against the model and seq == deltas applied + 1,
  // then pushes the rows chunk by chunk and sets the bias.
  struct DeltaResult { long long n_moved = 0, bytes = 0; std::string file; };
  void prepare_publish(const std::string &prefix, const std::string &fmt, long long seq_done);
  DeltaResult publish_delta(const std::string &prefix, const std::string &fmt, long long seq);
  DeltaResult apply_delta(const std::string &path);
  long long deltas_applied() const { return deltas_applied_; }

  void pull_linear();   // device -> bias, lin_w (from the shards that own them)
  void push_linear();
  void pull_weights();  // device -> bias, lin_w and the rows of vec_w that are mirrored
  void push_weights();  // bias, lin_w and the mirrored rows of vec_w -> device
  bool has_zero_weights();

  ModelType model_type;
  float bias = 0.0f;
  std::vector<float> lin_w;
  LatentMirror vec_w;  // [n_feats][row_len], lazy; empty for LR

  // features per chunk when a whole model is streamed (files, has_zero_weights, pull_all)
  size_t stream_chunk() const;
  void get_latent_rows(int component, size_t first, size_t count, float *out);  // 0 = w, 1 = n, 2 = z
  void set_latent_rows(int component, size_t first, size_t count, const float *in);

  ffm_engine *engine() { return eng_; }
  int64_t row_len() const { return row_len_; }

 protected:
  int n_feats, n_fields, n_factors;
  int64_t row_len_ = 0;
  ffm_engine *eng_ = nullptr;   // the engine (shard 0 of the group when there is one)
  // --n_gpus > 1: one field-pair shard engine per device, RCCL all-reduce of the partial logits per
  // block (include/ffm_engine.h: ffm_group_*)
  ffm_group *grp_ = nullptr;
  int n_gpus_ = 1;
  int metrics_mask_ = 0;
  int keyed_mask_ = 0, keyed_field_ = -1;  // --auc_key_field (-1: not asked for)
  size_t curve_variants_ = 0;               // enable_pair_curve: its cuts + 1 (0: not enabled)
  long long keyed_rows_ = 0;               // --auc_key_rows
  std::vector<int32_t> lin_owner_of_field_;  // [n_fields] shard that owns a field's linear terms
  int bias_owner_ = 0;
  double eval_loss_pending_ = 0.0;  // group: evaluation blocks are predicted synchronously
  std::vector<std::pair<float *, size_t>> pinned_scores_;  // pin_scores() ranges (floats)
  ffm_engine *shard(int r) const;
  // the field that owns a model id: a search in the ranges (uniform ranges: one divide; no ranges: 0)
  int field_of(int feat) const {
    if (per_field_ > 0) return std::min(feat / per_field_, n_fields - 1);
    if (field_start_.size() < 2) return 0;
    return static_cast<int>(std::upper_bound(field_start_.begin() + 1, field_start_.end() - 1, feat) - (field_start_.begin() + 1));
  }
  int per_field_ = 0;  // ids per field under --field_ranges uniform
  std::vector<int32_t> field_start_;  // [n_fields + 1] the fields' id ranges (--field_ranges uniform | counted | @FILE), or empty
  // what the engine was created from, as far as it decides a fresh model's contents (checkpoints)
  uint64_t seed_ = 0;
  float init_mean_ = 0.0f, init_stddev_ = 0.0f;
  int32_t flags_ = 0;
  bool serving_ = false;   // --serve_weights f32 | f16: a serving engine behind this model (prediction only)
  std::string serve_fmt_ = "none";  // ... its format
  // serving deltas: the shadow serving engine of publish_delta (null until asked for), its format, the deltas it
  // has behind it; deltas_applied_: those apply_delta has pushed into this (serving) model
  ffm_engine *shadow_ = nullptr;
  std::string shadow_fmt_;
  long long shadow_seq_ = 0, deltas_applied_ = 0;
  int device_ = 0;
  void make_shadow(const std::string &fmt);
  DeltaResult apply_delta_to(ffm_engine *e, const std::string &fmt, const std::string &path, long long want_seq);
  bool hash_ids_ = false;  // --hash_feats: ids >= n_feats are not erased on the host, the device hashes them
  bool compact_rows_ = false;  // --compact_rows: blocks go without the arrays their facts make redundant
  long long compact_blocks_ = 0, compact_no_val_ = 0, compact_no_field_ = 0;
  struct Wire { const int32_t *field; const float *val; };
  Wire wire(const CsrBlock &b, bool staged);  // the two optional arrays of one engine call (counted)
  CsrBlock one_;  // scratch for the one-row shims
  // engine capacities chosen at construction; blocks beyond max_nnz_ are split into several
  // engine calls (each still a block in row order), a single row beyond max_row_nnz_ is an error
  int max_rows_ = 0, max_nnz_ = 0, max_row_nnz_ = 0;
  long long handed_over_ = 0;  // blocks passed to the engine's pipelined entry points so far
  CsrBlock part_;
  // calls `fn(sub-block)` for consecutive row ranges of blk that fit the engine
  template <typename Fn> void for_each_fitting(const CsrBlock &blk, Fn fn);
  void check_resident(const ffm_rows_block &blk) const;
};

class LR : public FtrlModel {
 public:
  explicit LR(const config_options &opt) : FtrlModel(opt, FFM_MODEL_LR) {}
};
class FM : public FtrlModel {
 public:
  explicit FM(const config_options &opt) : FtrlModel(opt, FFM_MODEL_FM) {}
};
class FFM : public FtrlModel {
 public:
  explicit FFM(const config_options &opt) : FtrlModel(opt, FFM_MODEL_FFM) {}
  void remove_out_range(feat_vec &feats) override;  // also filters the field (ffm.cpp:30-36)
};

std::unique_ptr<FtrlModel> make_model(const config_options &opt);  // throws std::invalid_argument

// loss(int y, double logit), src/include/eval/loss.h:8-12
double loss(int y, double logit);

}  // namespace ftrl
