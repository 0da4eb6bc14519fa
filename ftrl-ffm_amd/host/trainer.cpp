#include "trainer.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <mutex>
#include <numeric>
#include <random>
#include <stdexcept>
#include <thread>

#include "importance.h"
#include "pair_mask.h"
#include "score_writer.h"

namespace ftrl {

using timer = std::chrono::steady_clock;
static double seconds_since(timer::time_point t0) {
  return std::chrono::duration<double>(timer::now() - t0).count();
}

void print_auc_line(FtrlModel &m, int epoch, int channel) {
  const ffm_metrics r = m.read_metrics(channel, true);
  std::printf("epoch %d %s auc: %.6lf (+-%.1e)\n", epoch, channel == FFM_METRIC_TRAIN ? "train" : "eval", r.auc, r.auc_slack);
  print_gauc_line(m, epoch, channel);
}

void print_gauc_line(FtrlModel &m, int epoch, int channel) {
  if (!m.keyed_metrics_on(channel)) return;
  const ffm_keyed_metrics r = m.read_keyed_metrics(channel, true);
  std::printf("epoch %d %s gauc: %.6lf (%lld keys, %lld mixed, %lld of %lld rows; %lld unkeyed, %lld over capacity, %lld nan)\n", epoch,
              channel == FFM_METRIC_TRAIN ? "train" : "eval", r.gauc, static_cast<long long>(r.n_keys),
              static_cast<long long>(r.n_keys_mixed), static_cast<long long>(r.n_rows_mixed), static_cast<long long>(r.n_rows),
              static_cast<long long>(r.n_unkeyed), static_cast<long long>(r.n_overflow), static_cast<long long>(r.n_nan));
}

void refresh_and_print(FtrlModel &m, long long epoch) {
  const ffm_refresh_stats r = m.refresh_weights();
  std::printf("epoch %lld weights: linear %lld live, %lld nonzero, %lld moved; latent %lld live, %lld nonzero, %lld moved\n", epoch,
              static_cast<long long>(r.lin_live), static_cast<long long>(r.lin_nonzero), static_cast<long long>(r.lin_moved),
              static_cast<long long>(r.lat_live), static_cast<long long>(r.lat_nonzero), static_cast<long long>(r.lat_moved));
}

void run_importance(const config_options &opt, FtrlModel &m, FtrlModel::Ablation kind) {
  const bool want_auc = opt.metrics == "auc", pairs = kind == FtrlModel::Ablation::Pairs;
  if (want_auc && pairs) {
    print_pair_histogram_memory(stdout, opt.n_fields);
    std::fflush(stdout);  // (the line is there when the allocation is refused)
  }
  m.enable_ablation(kind, want_auc);
  CsrStream stream(opt.eval_path, opt.file_type, opt.thread_num);
  const size_t batch = static_cast<size_t>(std::max(1, opt.batch_size));
  std::vector<double> loss(m.ablation_variants(kind), 0.0);
  CsrBlock blk;
  unsigned long long rows = 0;
  for (;;) {
    const size_t got = stream.next(batch, blk);
    if (got == 0) break;
    m.predict_ablated_block(kind, blk, loss);
    rows += got;
  }
  std::vector<ffm_metrics> auc;
  if (want_auc) auc = m.read_ablation_metrics(kind, true);
  (pairs ? print_pair_importance : print_field_importance)(stdout, opt.n_fields, rows, loss, want_auc ? &auc : nullptr);
  // --pair_curve LIST|auto [--pair_loss_budget T --pair_mask_out FILE]: the ranking as a ladder, one more pass
  if (pairs && !opt.pair_curve.empty()) run_pair_curve(opt, m, loss);
  // --pair_keep N --pair_mask_out FILE: the pass's answer as a mask file (pair_mask.h: the rule and the format)
  if (pairs && opt.pair_keep >= 0) {
    double smallest = 0.0;
    const PairList kept = select_pairs(opt.n_fields, loss, opt.pair_keep, &smallest);
    write_pair_mask(opt.pair_mask_out, opt.n_fields, kept);
    std::printf("pair mask: kept %zu of %d pairs, smallest kept delta %+.6lf -> %s\n", kept.size(), pair_count(opt.n_fields),
                smallest / (rows ? static_cast<double>(rows) : 1.0), opt.pair_mask_out.c_str());
  }
}

void run_pair_curve(const config_options &opt, FtrlModel &m, const std::vector<double> &pair_loss) {
  const bool want_auc = opt.metrics == "auc";
  const std::vector<int> &keep = opt.pair_curve_keep;  // ascending, no duplicates (cmd_option)
  // level = a pair's rank under select_pairs' own rule, so cut N keeps the pairs --pair_keep N would write
  const std::vector<uint16_t> level = pair_curve_levels(opt.n_fields, rank_pairs(opt.n_fields, pair_loss));
  m.enable_pair_curve(level, std::vector<int32_t>(keep.begin(), keep.end()), want_auc);
  CsrStream stream(opt.eval_path, opt.file_type, opt.thread_num);
  const size_t batch = static_cast<size_t>(std::max(1, opt.batch_size));
  std::vector<double> loss(keep.size() + 1, 0.0);
  CsrBlock blk;
  unsigned long long rows = 0;
  for (;;) {
    const size_t got = stream.next(batch, blk);
    if (got == 0) break;
    m.predict_curve_block(blk, loss);
    rows += got;
  }
  std::vector<ffm_metrics> auc;
  if (want_auc) auc = m.read_curve_metrics(true);
  print_pair_curve(stdout, opt.n_fields, rows, keep, loss, want_auc ? &auc : nullptr);
  if (!opt.pair_loss_budget_set) return;
  const int at = pick_by_budget(keep, loss, rows, opt.pair_loss_budget);
  const double n = rows ? static_cast<double>(rows) : 1.0;
  if (at < 0) {
    std::printf("pair mask: no listed number of pairs has a loss delta within budget %.6lf: nothing written\n", opt.pair_loss_budget);
    std::fflush(stdout);
    throw std::runtime_error("--pair_loss_budget: no listed number of pairs meets the budget");
  }
  const size_t i = static_cast<size_t>(at);
  const PairList kept = select_pairs(opt.n_fields, pair_loss, keep[i]);
  write_pair_mask(opt.pair_mask_out, opt.n_fields, kept);
  std::printf("pair mask: kept %zu of %d pairs, loss delta %+.6lf within budget %.6lf -> %s\n", kept.size(), pair_count(opt.n_fields),
              (loss[i] - loss.back()) / n, opt.pair_loss_budget, opt.pair_mask_out.c_str());
}

void load_pair_mask(const config_options &opt, FtrlModel &m) {
  const std::string file = opt.pair_mask.substr(1);  // (@FILE: cmd_option checked the form)
  const PairList kept = read_pair_mask(file, opt.n_fields);
  m.set_pair_mask(pair_mask_words(opt.n_fields, kept));
  std::printf("pair mask: %zu of %d pairs kept, from %s\n", kept.size(), pair_count(opt.n_fields), file.c_str());
}

void publish_and_print(FtrlModel &m, const std::string &prefix, const std::string &fmt, long long epoch, long long n_feats) {
  const FtrlModel::DeltaResult r = m.publish_delta(prefix, fmt, epoch);
  std::printf("epoch %lld published: %lld of %lld features moved, %lld bytes -> %s\n", epoch, r.n_moved, n_feats, r.bytes, r.file.c_str());
}

// ---------------- offline: data in memory, seeded shuffle per epoch ----------------

FtrlOffline::FtrlOffline(const config_options &opt)
    : model_ptr(make_model(opt)), n_epochs(opt.epoch), n_threads(opt.thread_num), seed_(opt.seed),
      sched_(opt.batch_size, opt.batch_ramp < 0 ? ffm_engine_default_batch_ramp(opt.w_alpha) : opt.batch_ramp) {
  // the files go straight into CSR (csr_reader.h); the Sample-based readers exist for callers
  // that use one_epoch(std::vector<Sample>&, ...) as the reference's tests do
  train_data_loader = std::make_unique<Reader>(opt.file_type);
  if (!opt.train_path.empty()) {  // (--n_epochs 0 needs no training file)
    std::printf("Loading data from file: %s\n", opt.train_path.c_str());
    const auto t0 = timer::now();
    train_csr_ = load_csr(opt.train_path, opt.file_type, n_threads);
    std::printf("Total number of samples loaded: %zu\nparsing data time: %.4lfs\n",
                train_csr_.n_rows(), seconds_since(t0));
  }
  if (!opt.eval_path.empty()) {
    eval_data_loader = std::make_unique<Reader>(opt.file_type);
    eval_csr_ = load_csr(opt.eval_path, opt.file_type, n_threads);
    has_eval_ = true;
  }
  metrics_ = opt.metrics == "auc";
  if (metrics_) model_ptr->enable_metrics(true, true);
  refresh_ = opt.refresh_weights;
  publish_ = opt.publish_path;
  publish_fmt_ = opt.publish_weights;
  n_feats_ = opt.n_feats;
}

FtrlOffline::~FtrlOffline() = default;

static void check_weight_rows(const SampleWeights &w, size_t rows) {
  if (!w.file.empty() && w.file.size() != rows)
    throw std::runtime_error("sample weights: " + std::to_string(w.file.size()) + " weights for " + std::to_string(rows) +
                             " training rows");
}
void FtrlOffline::set_sample_weights(SampleWeights w) {
  check_weight_rows(w, train_csr_.n_rows());
  weights_ = std::move(w);
}
// mean of a weighted epoch: sum(w * loss) / sum(w); no weight at all has no mean
static double weighted_mean(double loss_sum, double weight_sum) {
  return weight_sum > 0.0 ? loss_sum / weight_sum : std::numeric_limits<double>::quiet_NaN();
}

// ---------------- the ring of page-locked blocks ----------------

BlockRing::~BlockRing() {
  for (auto &b : ring_) model_->unpin_block(b);
}
bool BlockRing::ready() {
  if (tried_) return !ring_.empty();
  tried_ = true;
  ring_.resize(kRing);
  seq_.assign(kRing, 0);
  for (int i = 0; i < kRing; i++)
    if (!model_->pin_block(ring_[i], with_weights_)) {  // no page-locked memory to be had: the copying path
      for (int j = 0; j < i; j++) model_->unpin_block(ring_[j]);
      ring_.clear();
      return false;
    }
  return true;
}
CsrBlock &BlockRing::acquire() {
  while (model_->blocks_pulled() < seq_[slot_]) std::this_thread::yield();
  return ring_[slot_];
}

// One pass over a CSR file image: training visits the rows in a seeded shuffle, block by block;
// evaluation in file order.  Mean of loss(y, logit) over all rows.
double FtrlOffline::csr_epoch(const CsrData &d, bool train) {
  const size_t total = d.n_rows();
  if (total == 0) return 0.0;
  std::vector<int> indices;
  if (train) {
    indices.resize(total);
    std::iota(indices.begin(), indices.end(), 0);
    std::shuffle(indices.begin(), indices.end(), std::mt19937_64{seed_ + (++epoch_no_)});
  }
  double total_loss = 0.0, weight_sum = 0.0;
  const bool weighted = train && weights_.on;
  CsrBlock blk;
  if (!ring_) ring_ = std::make_unique<BlockRing>(model_ptr.get(), weights_.on);
  const bool ring = ring_->ready();
  size_t pos = 0;
  while (pos < total) {
    const size_t rows = std::min<size_t>(train ? sched_.next_block_rows() : sched_.max_block_rows(), total - pos);
    // both passes are pipelined: this block is uploaded (and, training, grouped) while the previous
    // ones run and the next one is gathered here -- straight into page-locked memory when there is a
    // ring entry it fits (the device then pulls it from there; the entry is reused once it has)
    const size_t nnz = train ? d.gather_nnz(indices.data() + pos, rows)
                             : static_cast<size_t>(d.row_ptr[pos + rows] - d.row_ptr[pos]);
    if (ring && rows <= ring_->row_capacity() && nnz <= ring_->nnz_capacity()) {
      CsrBlock &rb = ring_->acquire();
      if (train) d.gather(indices.data() + pos, rows, rb, n_threads); else d.slice(pos, pos + rows, rb);
      if (weighted) weight_sum += weights_.fill(rb, indices.data() + pos, 0);
      ring_->handed_over(train ? model_ptr->train_block_pinned(rb) : model_ptr->predict_block_async(rb, true));
    } else if (train) {
      d.gather(indices.data() + pos, rows, blk, n_threads);
      if (weighted) weight_sum += weights_.fill(blk, indices.data() + pos, 0);
      model_ptr->train_block_async(blk);
    } else {
      d.slice(pos, pos + rows, blk);
      model_ptr->predict_block_async(blk, false);
    }
    if (train) sched_.consumed(static_cast<int>(rows));
    pos += rows;
  }
  total_loss = train ? model_ptr->train_flush() : model_ptr->eval_flush();
  if (weighted) return weighted_mean(total_loss, weight_sum);
  return total_loss / static_cast<double>(total);
}

void FtrlOffline::train() {
  const int first = resumed_epochs_;  // (epochs a resumed run has behind it: the numbering continues; else 0)
  for (int i = first + 1; i <= first + n_epochs; i++) {
    const auto t0 = timer::now();
    const double train_loss = csr_epoch(train_csr_, true);
    std::printf("epoch %d train time: %.4lfs, train loss: %.4lf\n", i, seconds_since(t0), train_loss);
    if (metrics_) print_auc_line(*model_ptr, i, FFM_METRIC_TRAIN);
    if (refresh_) refresh_and_print(*model_ptr, i);
    if (!publish_.empty()) publish_and_print(*model_ptr, publish_, publish_fmt_, i, n_feats_);
    if (has_eval_) evaluate(i);
  }
}

void FtrlOffline::evaluate(int epoch) {
  const auto t0 = timer::now();
  const double eval_loss = csr_epoch(eval_csr_, false);
  std::printf("epoch %d eval time: %.4lfs, eval loss: %.4lf\n", epoch, seconds_since(t0), eval_loss);
  if (metrics_) print_auc_line(*model_ptr, epoch, FFM_METRIC_EVAL);
}

// One pass over `samples`: training visits them in a seeded shuffle (the reference shuffles from
// std::random_device, ftrl_offline.cpp:67-71), block by block; evaluation in order.  Returns the
// mean of loss(y, logit) over all rows, as ftrl_offline.cpp:101-102.
double FtrlOffline::one_epoch(std::vector<Sample> &samples, bool train, bool /*use_pool*/) {
  const size_t total = samples.size();
  if (total == 0) return 0.0;
  std::vector<int> indices(total);
  std::iota(indices.begin(), indices.end(), 0);
  if (train) std::shuffle(indices.begin(), indices.end(), std::mt19937_64{seed_ + (++epoch_no_)});
  double total_loss = 0.0;
  CsrBlock blk;
  size_t pos = 0;
  while (pos < total) {
    const size_t rows = std::min<size_t>(train ? sched_.next_block_rows() : sched_.max_block_rows(), total - pos);
    blk.clear();
    for (size_t r = 0; r < rows; r++) blk.push(samples[indices[pos + r]]);
    if (train) model_ptr->train_block_async(blk); else total_loss += model_ptr->predict_block(blk, false);
    if (train) sched_.consumed(static_cast<int>(rows));
    pos += rows;
  }
  if (train) total_loss = model_ptr->train_flush();
  return total_loss / static_cast<double>(total);
}

// ---------------- online: streaming from the file, file order ----------------

FtrlOnline::FtrlOnline(const config_options &opt)
    : model_ptr(make_model(opt)), n_epochs(opt.epoch), cmd_(opt.cmd),
      sched_(opt.batch_size, opt.batch_ramp < 0 ? ffm_engine_default_batch_ramp(opt.w_alpha) : opt.batch_ramp) {
  metrics_ = opt.metrics == "auc";
  if (metrics_) model_ptr->enable_metrics(true, true);
  refresh_ = opt.refresh_weights;
  publish_ = opt.publish_path;
  publish_fmt_ = opt.publish_weights;
  n_feats_ = opt.n_feats;
  if (!cmd_) {
    if (!opt.train_path.empty() && opt.device_rows && opt.epoch > 0) {
      FtrlModel *m = model_ptr.get();
      train_rows_ = std::make_unique<RowStream>(opt.train_path, opt.file_type, opt.thread_num, opt.device, m->block_rows_capacity(),
                                                m->block_nnz_capacity(), "train", [m] { return m->blocks_pulled(); });
    } else if (!opt.train_path.empty())  // (--n_epochs 0 needs no training file)
      train_stream_ = std::make_unique<CsrStream>(opt.train_path, opt.file_type, opt.thread_num);
    if (!opt.eval_path.empty()) {
      evaluator = std::make_unique<Evaluator>(opt);
      evaluator->load_trained_model(model_ptr);
    }
  }
}

void FtrlOnline::set_sample_weights(SampleWeights w) { weights_ = std::move(w); }

// One pass over the training file in FILE ORDER (the reference's deterministic order at one
// thread): worker threads parse chunks of <= 20 000 lines ahead (parse time is inside
// the timed region, as in the reference's online mode), the rows are cut into blocks by the
// block-size ramp, gathered in page-locked ring entries and handed to the engine, which uploads
// and groups block t+2 while block t trains.
void FtrlOnline::run_train_file() {
  if (train_rows_) {  // --device_rows true: the same blocks, cut in HBM
    unsigned long long rows = 0, next_report = 1000000;
    for (;;) {
      ffm_rows_block blk{};
      const size_t got = train_rows_->next(static_cast<size_t>(sched_.next_block_rows()), &blk);
      if (got == 0) break;
      model_ptr->train_block_resident(blk);
      train_rows_->handed_over(blk);
      sched_.consumed(static_cast<int>(got));
      rows += got;
      if (rows >= next_report) {  // pc_task.cpp:47-49
        std::printf("%llu lines finished...\n", next_report);
        next_report += 1000000;
      }
    }
    loss_sum_ = model_ptr->train_flush();
    loss_rows_ = rows;
    weight_sum_ = 0.0;
    train_rows_->rewind();
    return;
  }
  if (!ring_) ring_ = std::make_unique<BlockRing>(model_ptr.get(), weights_.on);
  const bool ring = ring_->ready();
  CsrBlock blk;
  unsigned long long rows = 0, next_report = 1000000;
  double weight_sum = 0.0;
  // (the rows come in file order: row j of a block is row `rows + j` of the file)
  auto weigh = [&](CsrBlock &b, size_t got) {
    if (!weights_.on) return;
    if (!weights_.file.empty() && rows + got > weights_.file.size())
      throw std::runtime_error("sample weights: the training file has more rows than the weight file has lines");
    weight_sum += weights_.fill(b, nullptr, static_cast<size_t>(rows));
  };
  for (;;) {
    const size_t want = static_cast<size_t>(sched_.next_block_rows());
    size_t got;
    if (ring) {
      CsrBlock &rb = ring_->acquire();
      got = train_stream_->next(std::min(want, ring_->row_capacity()), rb, ring_->nnz_capacity(), true);
      if (got == 0) break;
      weigh(rb, got);
      ring_->handed_over(model_ptr->train_block_pinned(rb));
    } else {
      got = train_stream_->next(want, blk);
      if (got == 0) break;
      weigh(blk, got);
      model_ptr->train_block_async(blk);
    }
    sched_.consumed(static_cast<int>(got));
    rows += got;
    if (rows >= next_report) {  // pc_task.cpp:47-49
      std::printf("%llu lines finished...\n", next_report);
      next_report += 1000000;
    }
  }
  loss_sum_ = model_ptr->train_flush();
  loss_rows_ = rows;
  weight_sum_ = weight_sum;
  train_stream_->rewind();
}

double FtrlOnline::get_loss() {
  double r = loss_rows_ ? loss_sum_ / static_cast<double>(loss_rows_) : 0.0;
  if (weights_.on && loss_rows_) r = weighted_mean(loss_sum_, weight_sum_);
  loss_sum_ = 0.0;
  loss_rows_ = 0;
  weight_sum_ = 0.0;
  return r;
}

void FtrlOnline::train() {
  if (cmd_) return;  // stdin mode is a TODO stub in the reference too (ftrl_online.cpp:55-57)
  for (int n = 0; n < n_epochs; n++) {
    const auto t0 = timer::now();
    run_train_file();
    passes_++;
    const int i = static_cast<int>(resumed_epochs_) + n + 1;  // (a resumed run's numbering continues; else 1..n_epochs)
    const double train_loss = get_loss();
    std::printf("epoch %d train time: %.4lfs, train loss: %.4lf\n", i, seconds_since(t0), train_loss);
    if (metrics_) print_auc_line(*model_ptr, i, FFM_METRIC_TRAIN);
    if (refresh_) refresh_and_print(*model_ptr, i);
    if (!publish_.empty()) publish_and_print(*model_ptr, publish_, publish_fmt_, i, n_feats_);
    if (evaluator) evaluate(i);
  }
}

void FtrlOnline::evaluate(int epoch) {
  if (!evaluator) return;
  const auto t0 = timer::now();
  evaluator->run();
  const double eval_loss = evaluator->get_loss();
  std::printf("epoch %d eval time: %.4lfs, eval loss: %.4lf\n", epoch, seconds_since(t0), eval_loss);
  if (metrics_) {
    double slack = 0.0;
    const double auc = evaluator->get_auc(&slack);
    std::printf("epoch %d eval auc: %.6lf (+-%.1e)\n", epoch, auc, slack);
    print_gauc_line(*model_ptr, epoch, FFM_METRIC_EVAL);  // (the evaluator scores with this model)
  }
}

// ---------------- Evaluator ----------------

Evaluator::Evaluator(const config_options &opt)
    : stream_(opt.device_rows ? nullptr : std::make_unique<CsrStream>(opt.eval_path, opt.file_type, opt.thread_num)),
      batch_(std::max(1, opt.batch_size)), want_auc_(opt.metrics == "auc") {
  if (opt.device_rows) {
    rows_path_ = opt.eval_path;
    rows_type_ = opt.file_type;
    rows_threads_ = opt.thread_num;
    rows_device_ = opt.device;
  }
}
Evaluator::~Evaluator() = default;

void Evaluator::load_trained_model(std::shared_ptr<FtrlModel> &train_model) {  // evaluate.cpp:35-37
  eval_model = train_model;
  // (--metrics auc: the eval channel on; whatever the owner of the model set for training stays)
  if (want_auc_ && !eval_model->metrics_on(FFM_METRIC_EVAL)) eval_model->enable_metrics(true, eval_model->metrics_on(FFM_METRIC_TRAIN));
  ring_ = std::make_unique<BlockRing>(eval_model.get());
  if (!rows_path_.empty()) {  // --device_rows true (the blocks' capacities are the model's)
    FtrlModel *m = eval_model.get();
    row_stream_ = std::make_unique<RowStream>(rows_path_, rows_type_, rows_threads_, rows_device_, m->block_rows_capacity(), m->block_nnz_capacity(),
                                        "eval", [m] { return m->blocks_pulled(); });
  }
}

void Evaluator::run() {
  if (!eval_model) throw std::logic_error("Evaluator::run before load_trained_model");
  if (row_stream_) {  // --device_rows true: the same blocks, cut in HBM
    unsigned long long rows = 0;
    for (;;) {
      ffm_rows_block blk{};
      const size_t got = row_stream_->next(static_cast<size_t>(batch_), &blk);
      if (got == 0) break;
      eval_model->predict_block_resident(blk);
      row_stream_->handed_over(blk);
      rows += got;
    }
    loss_sum_ = eval_model->eval_flush();
    rows_ = rows;
    row_stream_->rewind();
    return;
  }
  const bool ring = ring_->ready();
  CsrBlock blk;
  unsigned long long rows = 0;
  for (;;) {
    size_t got;
    if (ring) {
      CsrBlock &rb = ring_->acquire();
      got = stream_->next(std::min<size_t>(batch_, ring_->row_capacity()), rb, ring_->nnz_capacity(), true);
      if (got == 0) break;
      ring_->handed_over(eval_model->predict_block_async(rb, true));
    } else {
      got = stream_->next(static_cast<size_t>(batch_), blk);
      if (got == 0) break;
      eval_model->predict_block_async(blk, false);
    }
    rows += got;
  }
  loss_sum_ = eval_model->eval_flush();
  rows_ = rows;
  stream_->rewind();
}

double Evaluator::get_auc(double *slack) {
  if (!eval_model) throw std::logic_error("Evaluator::get_auc before load_trained_model");
  const ffm_metrics r = eval_model->read_metrics(FFM_METRIC_EVAL, true);
  if (slack) *slack = r.auc_slack;
  return r.auc;
}

double Evaluator::get_loss() {
  const double r = rows_ ? loss_sum_ / static_cast<double>(rows_) : 0.0;
  loss_sum_ = 0.0;
  rows_ = 0;
  return r;
}

// ---------------- Scorer ----------------

Scorer::Scorer(const config_options &opt, FtrlModel *model)
    : model_(model), stream_(opt.device_rows ? nullptr : std::make_unique<CsrStream>(opt.predict_path, opt.file_type, opt.thread_num)),
      out_path_(opt.predict_out), batch_(std::max(1, opt.batch_size)), n_threads_(std::max(1, opt.thread_num)),
      prob_(opt.predict_prob) {
  if (opt.device_rows)
    row_stream_ = std::make_unique<RowStream>(opt.predict_path, opt.file_type, opt.thread_num, opt.device, model->block_rows_capacity(),
                                        model->block_nnz_capacity(), "predict", [model] { return model->blocks_pulled(); });
}
Scorer::~Scorer() = default;

unsigned long long Scorer::run() {
  std::FILE *f = std::fopen(out_path_.c_str(), "wb");
  if (!f) throw std::runtime_error("cannot open " + out_path_ + " for writing");
  BlockRing ring(model_);
  const bool pinned_rows = !row_stream_ && ring.ready();
  // the ring of score buffers: entry i % kScoreRing carries block i from its hand-over to its write
  struct Entry {
    std::vector<float, PageAllocator<float>> buf;
    bool pinned = false;
    size_t rows = 0;
    long long wait_for = 0;  // the ordinal blocks_scored() must reach; 0: the scores are already there
  };
  std::vector<Entry> ent(kScoreRing);
  for (auto &en : ent) {
    en.buf.resize(static_cast<size_t>(batch_));
    en.pinned = model_->pin_scores(en.buf.data(), en.buf.size());
  }
  std::mutex mu;
  std::condition_variable cv;
  size_t submitted = 0, written = 0;
  bool done = false;
  std::atomic<bool> give_up{false};
  bool write_failed = false;
  // (formatting is ~50 ns per score on one thread -- a fifth of the rate the device predicts at: a block is
  // formatted in up to --n_threads slices side by side, then written in order)
  const int fmt_threads = std::max(1, n_threads_);
  std::thread writer([&] {
    std::vector<std::string> text(static_cast<size_t>(fmt_threads));
    for (size_t i = 0;; i++) {
      {
        std::unique_lock<std::mutex> lock(mu);
        cv.wait(lock, [&] { return submitted > i || done; });
        if (submitted <= i) return;
      }
      const Entry &en = ent[i % kScoreRing];
      // (the block's predict launch is deferred by one call: it is whole after the next hand-over, or
      // after the flush that ends the pass)
      while (en.wait_for > 0 && model_->blocks_scored() < en.wait_for) {
        if (give_up.load()) return;
        std::this_thread::sleep_for(std::chrono::microseconds(20));
      }
      const int slices = static_cast<int>(std::min<size_t>(static_cast<size_t>(fmt_threads), (en.rows + 1023) / 1024));
      const size_t per = slices > 0 ? (en.rows + static_cast<size_t>(slices) - 1) / static_cast<size_t>(slices) : 0;
#pragma omp parallel for schedule(static, 1) num_threads(slices) if (slices > 1)
      for (int t = 0; t < slices; t++) {
        const size_t lo = std::min(en.rows, per * static_cast<size_t>(t)), hi = std::min(en.rows, lo + per);
        text[static_cast<size_t>(t)].clear();
        append_scores(en.buf.data() + lo, hi - lo, text[static_cast<size_t>(t)]);
      }
      for (int t = 0; t < slices && !write_failed; t++)
        write_failed = std::fwrite(text[static_cast<size_t>(t)].data(), 1, text[static_cast<size_t>(t)].size(), f) != text[static_cast<size_t>(t)].size();
      {
        std::lock_guard<std::mutex> lock(mu);
        written = i + 1;
      }
      cv.notify_all();
    }
  });
  auto finish = [&](bool failed) {
    if (failed) give_up.store(true);
    {
      std::lock_guard<std::mutex> lock(mu);
      done = true;
    }
    cv.notify_all();
    writer.join();
    for (auto &en : ent)
      if (en.pinned) model_->unpin_scores(en.buf.data());
  };
  unsigned long long rows = 0;
  try {
    CsrBlock blk;
    for (size_t i = 0;; i++) {
      {  // entry i % kScoreRing is free once block i - kScoreRing is in the file
        std::unique_lock<std::mutex> lock(mu);
        cv.wait(lock, [&] { return written + kScoreRing > i; });
      }
      Entry &en = ent[i % kScoreRing];
      const CsrBlock *b = &blk;
      size_t got;
      if (row_stream_) {  // --device_rows true: the same blocks, cut in HBM; the score ring and the writer as they are
        if (!en.pinned) throw std::runtime_error("--device_rows true needs page-locked score buffers, and none could be had");
        ffm_rows_block rb{};
        got = row_stream_->next(static_cast<size_t>(batch_), &rb);
        if (got == 0) break;
        const long long ordinal = model_->predict_block_resident(rb, en.buf.data(), prob_);
        row_stream_->handed_over(rb);
        en.rows = got;
        en.wait_for = ordinal;
        {
          std::lock_guard<std::mutex> lock(mu);
          submitted = i + 1;
        }
        cv.notify_all();
        rows += got;
        continue;
      }
      if (pinned_rows) {
        CsrBlock &rb = ring.acquire();
        got = stream_->next(std::min<size_t>(batch_, ring.row_capacity()), rb, ring.nnz_capacity(), true);
        b = &rb;
      } else {
        got = stream_->next(static_cast<size_t>(batch_), blk);
      }
      if (got == 0) break;
      bool complete = false;
      const long long ordinal = model_->predict_block_async(*b, pinned_rows, en.buf.data(), prob_, &complete);
      if (pinned_rows) ring.handed_over(ordinal);
      en.rows = got;
      en.wait_for = complete ? 0 : ordinal;
      {
        std::lock_guard<std::mutex> lock(mu);
        submitted = i + 1;
      }
      cv.notify_all();
      rows += got;
    }
    model_->eval_flush();  // (launches the last block and waits; the labels' loss is not reported)
  } catch (...) {
    finish(true);
    std::fclose(f);
    throw;
  }
  finish(false);
  const bool closed = std::fclose(f) == 0;
  if (write_failed || !closed) throw std::runtime_error("writing " + out_path_ + " failed");
  if (row_stream_) row_stream_->rewind(); else stream_->rewind();
  return rows;
}

}  // namespace ftrl
