// trainer.h -- FtrlOffline / FtrlOnline / Evaluator over the block engine.
//
// Replaces the reference's per-sample thread pool and producer/consumer queue
// (src/task/ftrl_offline.cpp:63-103, src/task/ftrl_online.cpp:42-80, src/eval/evaluate.cpp:23-49,
// src/include/concurrent/*) with a mini-batch scheduler: rows are packed into CSR blocks on the
// host and handed to the engine one block at a time.  Same constructors, train(), evaluate(),
// has_zero_weights(), model_ptr and printed lines as the reference.
//
// Block-size ramp: block t holds min(batch_size, max(1, rows_seen / batch_ramp)) rows, so the
// staleness of the weights a row sees never exceeds 1/batch_ramp of the rows already learned
// from -- that keeps the epoch logloss within 1e-4 of the reference's strictly sequential loop
// (DESIGN.md "Batch semantics"; batch_ramp = 0 turns the ramp off; the default follows the learning
// rate: ffm_engine_default_batch_ramp(w_alpha), 32 at the reference's rates).
#pragma once
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "ftrl_model.h"
#include "csr_reader.h"
#include "csr_stream.h"
#include "reader.h"
#include "row_stream.h"
#include "sample_weights.h"

namespace ftrl {

class BlockScheduler {
 public:
  BlockScheduler(int batch_size, int batch_ramp) : batch_(batch_size), ramp_(batch_ramp) {}
  int next_block_rows() const {
    if (ramp_ <= 0) return batch_;
    const long long r = seen_ / ramp_;
    return static_cast<int>(std::min<long long>(batch_, std::max<long long>(1, r)));
  }
  int max_block_rows() const { return batch_; }  // evaluation has no staleness: full blocks
  void consumed(int rows) { seen_ += rows; }
  long long rows_seen() const { return seen_; }
  void restore(long long rows_seen) { seen_ = rows_seen; }  // a resumed run continues the ramp

 private:
  int batch_, ramp_;
  long long seen_ = 0;
};

// A ring of page-locked blocks the device pulls from in place (FtrlModel::train_block_pinned /
// predict_block_async): an entry is refilled once the engine has uploaded the block it carried.
class BlockRing {
 public:
  static constexpr int kRing = 6;
  // with_weights: the entries' weight arrays are page-locked too (training with sample weights)
  explicit BlockRing(FtrlModel *m, bool with_weights = false) : model_(m), with_weights_(with_weights) {}
  ~BlockRing();
  bool ready();                       // pins the entries on first use; false: no page-locked memory
  CsrBlock &acquire();                // the next entry, free to be refilled
  void handed_over(long long ordinal) { seq_[slot_] = ordinal; slot_ = (slot_ + 1) % kRing; }
  size_t row_capacity() { return ring_[0].row_ptr.capacity() - 1; }
  size_t nnz_capacity() { return ring_[0].feat.capacity(); }

 private:
  FtrlModel *model_;
  bool with_weights_ = false;
  std::vector<CsrBlock> ring_;
  std::vector<long long> seq_;
  int slot_ = 0;
  bool tried_ = false;
};

// Evaluator (reference src/include/eval/evaluate.h:18-33, src/eval/evaluate.cpp:7-54): streams the
// eval file through predict() and reports the mean logloss.  Here: chunks parsed by n_threads
// workers (CsrStream), blocks gathered in page-locked memory, uploaded and predicted pipelined
// (FtrlModel::predict_block_async).
class Evaluator {
 public:
  explicit Evaluator(const config_options &opt);
  ~Evaluator();
  void load_trained_model(std::shared_ptr<FtrlModel> &train_model);
  void run();          // one pass over the eval file (PcTask::run in the reference)
  double get_loss();   // mean loss of the last pass (resets it)
  // AUC of the last pass from the model's eval channel (resets the channel); *slack: the most the exact
  // rank AUC can differ.  The channel is turned on by --metrics auc (or FtrlModel::enable_metrics).
  double get_auc(double *slack = nullptr);

 private:
  std::shared_ptr<FtrlModel> eval_model;
  std::unique_ptr<CsrStream> stream_;
  std::unique_ptr<BlockRing> ring_;
  // --device_rows true: the file is read through these instead (row_stream.h; made by load_trained_model)
  std::unique_ptr<RowStream> row_stream_;
  std::string rows_path_, rows_type_;
  int rows_threads_ = 1, rows_device_ = 0;
  int batch_;
  bool want_auc_ = false;
  double loss_sum_ = 0.0;
  unsigned long long rows_ = 0;
};

// Scorer (--predict_data / --predict_out): streams a file through the model and writes one prediction
// per row, in file order.  Modelled on Evaluator: chunks parsed by n_threads workers (CsrStream), blocks
// gathered in the page-locked BlockRing, uploaded and predicted pipelined (FtrlModel::
// predict_block_async) -- with a small ring of page-locked score buffers which the device fills behind
// each block's predict kernel.  A writer thread waits for FtrlModel::blocks_scored(), formats the block
// (score_writer.h; in up to --n_threads slices side by side, never by the machine's core count) and
// appends it while the next blocks are parsed and predicted.  Memory is bounded by the two rings, never by the file.  The file's label
// column is parsed and ignored: nothing of the pass is reported but the rows.
// On a group (--n_gpus > 1) every block is predicted by the synchronous ffm_group_predict_batch.
class Scorer {
 public:
  static constexpr int kScoreRing = 6;
  Scorer(const config_options &opt, FtrlModel *model);
  ~Scorer();
  unsigned long long run();  // one pass over the file; returns the rows written

 private:
  FtrlModel *model_;
  std::unique_ptr<CsrStream> stream_;
  std::unique_ptr<RowStream> row_stream_;  // --device_rows true: instead of stream_
  std::string out_path_;
  int batch_, n_threads_;
  bool prob_;
};

// --metrics auc: the line that follows an epoch's loss line ("train" / "eval"); resets the channel.
void print_auc_line(FtrlModel &m, int epoch, int channel);
// --auc_key_field: the grouped-AUC line that follows it (nothing when the model keeps no keys); resets the capture.
void print_gauc_line(FtrlModel &m, int epoch, int channel);
// --refresh_weights true: FtrlModel::refresh_weights() and its line,
// `epoch N weights: linear L live, Z nonzero, M moved; latent L live, Z nonzero, M moved`.
// The tasks call it after each epoch's training, before that epoch's evaluation; main() where no epoch ran.
void refresh_and_print(FtrlModel &m, long long epoch);
// --field_importance true, --pair_importance true: one more pass over --eval_data through
// FtrlModel::predict_ablated_block (the host parser's blocks, the synchronous call, loss sums added in block order)
// and the kind's lines of importance.h; for the pairs with --metrics auc the histograms' memory is printed before
// FtrlModel::enable_ablation allocates it.
// With --pair_keep N --pair_mask_out FILE the pairs' pass then ranks them (pair_mask.h), writes the mask file and
// prints `pair mask: kept N of V pairs, smallest kept delta D -> FILE` (D per row, as the pairs' lines print it).
void run_importance(const config_options &opt, FtrlModel &m, FtrlModel::Ablation kind);
// --pair_curve LIST|auto, behind the pairs' pass (pair_loss: its V + 1 sums): ranks the pairs by select_pairs' rule,
// makes one more pass over --eval_data through FtrlModel::predict_curve_block with level = rank and the listed N as
// cuts (include/ffm_engine.h "Pruning curve"), and prints importance.h's `pair curve` lines.  With --pair_loss_budget T
// --pair_mask_out FILE it then writes the mask of the smallest listed N whose per-row loss delta is <= T and prints
// `pair mask: kept N of V pairs, loss delta D within budget T -> FILE`; when no listed N meets the budget it writes
// nothing, prints a line that says so and throws std::runtime_error (the run exits non-zero).
void run_pair_curve(const config_options &opt, FtrlModel &m, const std::vector<double> &pair_loss);
// --pair_mask @FILE: reads the file against the run's --n_fields, sets the mask on the loaded model
// (FtrlModel::set_pair_mask) and prints `pair mask: K of V pairs kept, from FILE`.
void load_pair_mask(const config_options &opt, FtrlModel &m);
// --publish_path: FtrlModel::publish_delta(prefix, fmt, epoch) and its line,
// `epoch N published: M of F features moved, B bytes -> FILE`
void publish_and_print(FtrlModel &m, const std::string &prefix, const std::string &fmt, long long epoch, long long n_feats);

class FtrlOffline {
 public:
  explicit FtrlOffline(const config_options &opt);
  ~FtrlOffline();
  void train();
  void evaluate(int epoch = 0);
  double one_epoch(std::vector<Sample> &samples, bool train, bool use_pool);
  bool has_zero_weights() { return model_ptr->has_zero_weights(); }
  // What a checkpoint carries beside the model so that an interrupted and resumed run IS the
  // uninterrupted one: the rows seen (block-size ramp) and the epochs done (the shuffle of epoch e is
  // seeded seed + e).  restore() before train(): --n_epochs then means that many MORE epochs.
  // (Without restore() nothing changes: train() numbers its epochs from 1 on every call.)
  FtrlModel::TrainProgress progress() const { return {sched_.rows_seen(), epoch_no_}; }
  void restore(const FtrlModel::TrainProgress &p) {
    sched_.restore(p.rows_seen);
    epoch_no_ = resumed_epochs_ = static_cast<int>(p.epochs_done);
  }

  // Per-row training weights (sample_weights.h), to be set before train(): row i of the training file
  // trains with w.of(i, label) -- the shuffled gather carries every row's weight along -- and the
  // `train loss` line becomes sum(w * loss) / sum(w) (nan when sum(w) is 0).  Evaluation is unweighted.
  void set_sample_weights(SampleWeights w);

  std::unique_ptr<FtrlModel> model_ptr;

 private:
  SampleWeights weights_;
  int n_epochs, n_threads;
  uint64_t seed_;
  int epoch_no_ = 0;        // training passes so far (the shuffle of pass e is seeded seed + e)
  int resumed_epochs_ = 0;  // epochs a checkpoint brought along: train() prints its epochs after them
  BlockScheduler sched_;
  bool metrics_ = false;    // --metrics auc
  bool refresh_ = false;    // --refresh_weights
  std::string publish_, publish_fmt_;  // --publish_path / --publish_weights
  long long n_feats_ = 0;
  std::unique_ptr<Reader> train_data_loader, eval_data_loader;  // API parity (data stays empty
                                                                // unless load_samples() is called)
  CsrData train_csr_, eval_csr_;                                // what train()/evaluate() walk
  bool has_eval_ = false;
  double csr_epoch(const CsrData &d, bool train);
  // Training and evaluation blocks are gathered straight into a ring of page-locked blocks which
  // the device pulls from: no host copy, three blocks in flight.
  std::unique_ptr<BlockRing> ring_;
};

class FtrlOnline {
 public:
  explicit FtrlOnline(const config_options &opt);
  void train();
  void evaluate(int epoch = 0);
  double get_loss();
  bool has_zero_weights() { return model_ptr->has_zero_weights(); }
  FtrlModel::TrainProgress progress() const { return {sched_.rows_seen(), resumed_epochs_ + passes_}; }  // (as FtrlOffline's)
  void restore(const FtrlModel::TrainProgress &p) { sched_.restore(p.rows_seen); resumed_epochs_ = p.epochs_done; }

  // Per-row training weights (sample_weights.h), to be set before train(): as FtrlOffline's, by the
  // row's number in the training file (file order).
  void set_sample_weights(SampleWeights w);

  std::shared_ptr<FtrlModel> model_ptr;
  std::unique_ptr<Evaluator> evaluator;  // (ftrl_online.h:31; null without --eval_data)

 private:
  void run_train_file();
  SampleWeights weights_;
  double weight_sum_ = 0.0;  // sum of the weights of the rows behind loss_sum_
  int n_epochs;
  long long passes_ = 0;          // passes over the training file made by this object
  long long resumed_epochs_ = 0;  // epochs a checkpoint brought along: train() prints its epochs after them
  bool cmd_;
  bool metrics_ = false;          // --metrics auc
  bool refresh_ = false;          // --refresh_weights
  std::string publish_, publish_fmt_;  // --publish_path / --publish_weights
  long long n_feats_ = 0;
  BlockScheduler sched_;
  std::unique_ptr<CsrStream> train_stream_;  // chunks of <= 20 000 lines parsed by n_threads workers
  std::unique_ptr<RowStream> train_rows_;    // --device_rows true: instead of train_stream_ (row_stream.h)
  std::unique_ptr<BlockRing> ring_;
  double loss_sum_ = 0.0;
  unsigned long long loss_rows_ = 0;
};

}  // namespace ftrl
