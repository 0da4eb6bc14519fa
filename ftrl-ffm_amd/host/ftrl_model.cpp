#include "ftrl_model.h"

#include "persist.h"
#include "serve_delta.h"

#include <algorithm>
#include <fstream>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

namespace ftrl {

static void check(int rc, const char *what) {
  if (rc != FFM_OK)
    throw std::runtime_error(std::string(what) + ": " + ffm_engine_last_error());
}

double loss(int y, double logit) {
  const double s = 1 / (1 + std::exp(-logit));
  return -y * std::log(s) - (1 - y) * std::log(1 - s);
}

FtrlModel::FtrlModel(const config_options &opt, int mt)
    : model_type(static_cast<ModelType>(mt)),
      n_feats(opt.n_feats), n_fields(opt.n_fields), n_factors(opt.n_factors) {
  ffm_engine_config cfg;
  ffm_engine_default_config(&cfg);
  cfg.model_type = mt;
  cfg.n_feats = opt.n_feats;
  cfg.n_fields = opt.n_fields;
  cfg.n_factors = opt.n_factors;
  cfg.w_alpha = opt.w_alpha;
  cfg.w_beta = opt.w_beta;
  cfg.w_l1 = opt.w_l1;
  cfg.w_l2 = opt.w_l2;
  cfg.init_mean = opt.init_mean;
  cfg.init_stddev = opt.init_stddev;
  cfg.seed = opt.seed;
  // The reference accepts rows of any length (feat_vec).  Here one row may hold up to 4096
  // entries (the row kernels stage a row in LDS) and one engine call up to max_nnz_ entries; a
  // denser block is fed as several calls (for_each_fitting), so --batch_size never has to be
  // chosen with the data's density in mind.
  max_rows_ = std::max(1, opt.batch_size);
  max_row_nnz_ = 4096;
  max_nnz_ = static_cast<int>(std::min<long long>(std::max<long long>(256ll * max_rows_, max_row_nnz_), 1ll << 28));
  cfg.max_batch_rows = max_rows_;
  cfg.max_batch_nnz = max_nnz_;
  cfg.max_row_nnz = max_row_nnz_;
  cfg.device_id = opt.device;
  if (opt.learn) cfg.flags |= FFM_FLAG_LEARN;
  // --hash_feats: the device hashes every id into range (include/ffm_engine.h "Hashed ids"); from here on
  // get/set_latent_rows, pull/push_linear, the model files and checkpoints speak MODEL (hashed) ids
  if (opt.hash_feats) cfg.flags |= FFM_FLAG_HASH_IDS;
  hash_ids_ = opt.hash_feats;
  // --normalize_rows: the device scales every row it is handed to unit length (include/ffm_engine.h "Normalised
  // rows"); the one-row shims below hand over the row of survivors, which gives what a block gives
  if (opt.normalize_rows) cfg.flags |= FFM_FLAG_NORM_ROWS;
  compact_rows_ = opt.compact_rows;
  keyed_field_ = opt.auc_key_field;  // (turned on with the AUC channels: enable_metrics)
  keyed_rows_ = opt.auc_key_rows;
  // --serve_weights: a serving engine (include/ffm_engine.h "Serving engines") -- the weights alone, rows of at
  // most 128 entries, prediction only; load_checkpoint then passes the saved w and nothing else
  serving_ = opt.serve_weights != "none";
  serve_fmt_ = opt.serve_weights;
  device_ = opt.device;
  if (serving_) {
    if (opt.serve_weights != "f32" && opt.serve_weights != "f16") throw std::invalid_argument("serve_weights: none, f32 or f16");
    if (opt.n_gpus > 1) throw std::invalid_argument("a serving engine is one whole model on one GPU (n_gpus == 1)");
    cfg.flags |= opt.serve_weights == "f16" ? FFM_FLAG_SERVE_F16 : FFM_FLAG_SERVE_F32;
    max_row_nnz_ = 128;
    max_nnz_ = static_cast<int>(std::min<long long>(std::max<long long>(256ll * max_rows_, max_row_nnz_), 1ll << 28));
    cfg.max_batch_nnz = max_nnz_;
    cfg.max_row_nnz = max_row_nnz_;
  }
  n_gpus_ = std::max(1, opt.n_gpus);
  seed_ = cfg.seed;
  init_mean_ = cfg.init_mean;
  init_stddev_ = cfg.init_stddev;
  flags_ = cfg.flags;
  int rc;
  const char *force_group = std::getenv("FFM_GROUP_RCCL");  // (a group of one: the RCCL path on a one-GPU box)
  if (n_gpus_ > 1 || (force_group && force_group[0] == '1' && mt == FFM_MODEL_FFM)) {
    // field-pair sharding needs field(i): --field_ranges uniform says field f owns the ids
    // [f * n_feats / n_fields, (f + 1) * n_feats / n_fields) (python/generate_data.py:272-306 lays
    // ids out per field); every shard then stores only the slots it owns
    if (mt != FFM_MODEL_FFM) throw std::invalid_argument("--n_gpus > 1 shards the FFM field pairs: model_type must be FFM");
    if (n_gpus_ > 1 && opt.field_ranges != "uniform")
      throw std::invalid_argument("--n_gpus > 1 needs --field_ranges uniform (per-field id ranges)");
    if (!opt.field_start.empty())
      throw std::invalid_argument("--field_ranges " + opt.field_ranges + " is for one engine: the group path takes uniform ranges only");
    std::vector<int32_t> fs(static_cast<size_t>(opt.n_fields) + 1);
    if (n_gpus_ <= 1) std::printf("FFM_GROUP_RCCL=1: one engine behind the group path (synchronous evaluation, RCCL all-reduce of one rank)\n");
    if (opt.field_ranges == "uniform") {
      if (opt.n_feats < opt.n_fields)
        throw std::invalid_argument("--field_ranges uniform needs n_feats >= n_fields (every field owns an id range)");
      per_field_ = opt.n_feats / opt.n_fields;
      for (int f = 0; f <= opt.n_fields; f++) fs[f] = f == opt.n_fields ? opt.n_feats : f * per_field_;
      if (n_gpus_ > 1 || opt.hash_feats) cfg.field_start = fs.data();  // (hashed: the ranges shape the mapping)
      field_start_ = fs;
    }
    std::vector<int32_t> devs(static_cast<size_t>(n_gpus_));
    const bool same = std::getenv("FTRL_SAME_DEVICE") != nullptr;  // one-GPU dry run of the orchestration
    for (int r = 0; r < n_gpus_; r++) devs[r] = same ? opt.device : opt.device + r;
    rc = ffm_group_create(&cfg, n_gpus_, devs.data(), &grp_);
    if (rc == FFM_E_INVALID) throw std::invalid_argument(ffm_engine_last_error());
    check(rc, "ffm_group_create");
    eng_ = ffm_group_engine(grp_, 0);
    lin_owner_of_field_.resize(static_cast<size_t>(opt.n_fields));
    int32_t bo = 0;
    check(ffm_engine_shard_plan(opt.n_fields, n_gpus_, n_gpus_ > 1 ? 1 : 0, nullptr, lin_owner_of_field_.data(), &bo), "ffm_engine_shard_plan");
    bias_owner_ = bo;
    std::printf("%d field-pair shards, collective: %s\n", n_gpus_, ffm_group_collective(grp_));
  } else {
    // one engine: --field_ranges uniform is a hint (the grouping sorts every field's id range by itself,
    // and a block whose rows are one entry per field in field order takes the short forms of the fold)
    // (--field_ranges counted | @FILE: the ranges main.cpp resolved, honoured where uniform ones are)
    std::vector<int32_t> fs;
    if (mt == FFM_MODEL_FFM && !opt.field_start.empty()) {
      if (opt.field_start.size() != static_cast<size_t>(opt.n_fields) + 1)
        throw std::invalid_argument("field ranges: " + std::to_string(opt.field_start.size()) + " values for " +
                                    std::to_string(opt.n_fields) + " fields (n_fields + 1 expected)");
      fs = opt.field_start;
      cfg.field_start = fs.data();
    } else if (mt == FFM_MODEL_FFM && opt.field_ranges == "uniform" && opt.n_feats >= opt.n_fields) {
      fs.resize(static_cast<size_t>(opt.n_fields) + 1);
      const int per = opt.n_feats / opt.n_fields;
      for (int f = 0; f <= opt.n_fields; f++) fs[f] = f == opt.n_fields ? opt.n_feats : f * per;
      cfg.field_start = fs.data();  // (copied by ffm_engine_create)
    }
    field_start_ = fs;
    rc = ffm_engine_create(&cfg, &eng_);
    if (rc == FFM_E_INVALID) throw std::invalid_argument(ffm_engine_last_error());
    check(rc, "ffm_engine_create");
  }
  // --min_count / --rare_ids: the keep-map main.cpp resolved -- training, serving and scoring engines alike fold by
  // it wherever they hash (include/ffm_engine.h "Rare ids"; a group is refused there as on the command line)
  if (!opt.rare_words.empty()) {
    rc = ffm_engine_set_rare_fold(eng_, opt.rare_map_bits, opt.rare_words.data());
    if (rc == FFM_E_INVALID || rc == FFM_E_UNSUPPORTED) throw std::invalid_argument(std::string("rare ids: ") + ffm_engine_last_error());
    check(rc, "ffm_engine_set_rare_fold");
  }
  // --bucket_fields / --buckets: the table main.cpp resolved, on training, serving and scoring engines alike
  // (include/ffm_engine.h "Value buckets")
  if (!opt.bucket_n_edges.empty()) {
    rc = ffm_engine_set_buckets(eng_, opt.bucket_n_edges.data(), opt.bucket_edges.data());
    if (rc == FFM_E_INVALID || rc == FFM_E_UNSUPPORTED) throw std::invalid_argument(std::string("value buckets: ") + ffm_engine_last_error());
    check(rc, "ffm_engine_set_buckets");
  }
  if (serving_)
    std::printf("serving weights: %s, %lld bytes of model\n", opt.serve_weights.c_str(), static_cast<long long>(ffm_engine_model_bytes(eng_)));
  row_len_ = ffm_engine_row_len(eng_);
  lin_w.resize(static_cast<size_t>(n_feats));
  vec_w.owner_ = this;
  vec_w.row_len_ = static_cast<size_t>(row_len_);
  vec_w.n_ = row_len_ > 0 ? static_cast<size_t>(n_feats) : 0;
  pull_linear();
}

FtrlModel::~FtrlModel() {
  if (shadow_) ffm_engine_destroy(shadow_);
  if (grp_) ffm_group_destroy(grp_); else ffm_engine_destroy(eng_);
}

ffm_engine *FtrlModel::shard(int r) const { return grp_ ? ffm_group_engine(grp_, r) : eng_; }

// bias and lin_w from their owners (one engine: the engine)
void FtrlModel::pull_linear() {
  if (!grp_) {
    check(ffm_engine_get_weights(eng_, &bias, lin_w.data(), nullptr), "ffm_engine_get_weights");
    return;
  }
  std::vector<float> tmp(lin_w.size());
  for (int r = 0; r < n_gpus_; r++) {
    float b = 0.0f;
    check(ffm_engine_get_weights(shard(r), &b, tmp.data(), nullptr), "ffm_engine_get_weights");
    if (r == bias_owner_) bias = b;
    for (size_t i = 0; i < tmp.size(); i++)
      if (lin_owner_of_field_[field_of(static_cast<int>(i))] == r) lin_w[i] = tmp[i];
  }
}
void FtrlModel::push_linear() {
  for (int r = 0; r < n_gpus_; r++)
    check(ffm_engine_set_weights(shard(r), &bias, lin_w.data(), nullptr), "ffm_engine_set_weights");
}

void FtrlModel::remove_out_range(feat_vec &feats) {  // ftrl_model.cpp:36-42
  feats.erase(std::remove_if(feats.begin(), feats.end(),
                             [&](const feat &f) {
                               const int i = std::get<1>(f);
                               return i < 0 || (i >= n_feats && !hash_ids_);  // (hashed into range on the device)
                             }),
              feats.end());
}

void FFM::remove_out_range(feat_vec &feats) {
  feats.erase(std::remove_if(feats.begin(), feats.end(),
                             [&](const feat &f) {
                               const auto [field, i, v] = f;
                               (void)v;
                               return field < 0 || i < 0 || field >= n_fields || (i >= n_feats && !hash_ids_);
                             }),
              feats.end());
}

float FtrlModel::train(feat_vec &features, int label) {
  remove_out_range(features);
  one_.clear();
  one_.push(Sample{features, label});
  one_.forget_facts();  // (the one-row shims hand over all five arrays, --compact_rows or not)
  float logit = 0.0f;
  train_block(one_, &logit);
  return logit;
}

float FtrlModel::predict(feat_vec &features, bool output_prob) {
  remove_out_range(features);
  one_.clear();
  one_.push(Sample{features, 0});
  one_.forget_facts();
  float out = 0.0f;
  predict_block(one_, output_prob, &out);
  return out;
}

// --compact_rows: the field and val arrays a block crosses PCIe with -- NULL where the block's facts
// (types.h: noted by whoever wrote its entries) say that the engine can write the array itself
// (include/ffm_engine.h: val == NULL is 1.0f; field == NULL is one entry per field in field order).
// staged: the call uploads through a staging slot -- the synchronous engine calls want an FFM block's field array.
FtrlModel::Wire FtrlModel::wire(const CsrBlock &b, bool staged) {
  Wire w{b.field.data(), b.val.data()};
  if (!compact_rows_) return w;
  compact_blocks_++;
  if (b.all_ones) { w.val = nullptr; compact_no_val_++; }
  if (staged && model_type == ModelType::FFM && b.one_entry_per_field(n_fields)) { w.field = nullptr; compact_no_field_++; }
  return w;
}

void FtrlModel::print_norm_rows() {
  if (!(flags_ & FFM_FLAG_NORM_ROWS)) return;
  int64_t rows = 0, left = 0;
  check(ffm_engine_norm_stats(eng_, 0, &rows, &left), "ffm_engine_norm_stats");
  std::printf("normalized rows: %lld scaled, %lld left as they came (zero or non-finite norm)\n", static_cast<long long>(rows - left),
              static_cast<long long>(left));
}

void FtrlModel::print_compact_rows() const {
  if (compact_rows_)
    std::printf("compact rows: %lld of %lld blocks without values, %lld without fields\n", compact_no_val_, compact_blocks_, compact_no_field_);
}

template <typename Fn>
void FtrlModel::for_each_fitting(const CsrBlock &blk, Fn fn) {
  const int n = blk.n_rows();
  if (n <= max_rows_ && blk.row_ptr[n] <= max_nnz_) {
    bool fits = true;
    for (int r = 0; r < n && fits; r++) fits = blk.row_ptr[r + 1] - blk.row_ptr[r] <= max_row_nnz_;
    if (fits) { fn(blk, 0); return; }
  }
  int r0 = 0;
  while (r0 < n) {
    int r1 = r0;
    while (r1 < n && r1 - r0 < max_rows_ && blk.row_ptr[r1 + 1] - blk.row_ptr[r0] <= max_nnz_) {
      if (blk.row_ptr[r1 + 1] - blk.row_ptr[r1] > max_row_nnz_)
        throw std::length_error("a row has " + std::to_string(blk.row_ptr[r1 + 1] - blk.row_ptr[r1]) +
                                " entries; this engine handles up to " + std::to_string(max_row_nnz_));
      r1++;
    }
    if (r1 == r0) throw std::length_error("a row exceeds the engine's block capacity");
    const int b = blk.row_ptr[r0], e = blk.row_ptr[r1];
    part_.row_ptr.resize(static_cast<size_t>(r1 - r0) + 1);
    for (int r = r0; r <= r1; r++) part_.row_ptr[r - r0] = blk.row_ptr[r] - b;
    part_.field.assign(blk.field.begin() + b, blk.field.begin() + e);
    part_.feat.assign(blk.feat.begin() + b, blk.feat.begin() + e);
    part_.val.assign(blk.val.begin() + b, blk.val.begin() + e);
    part_.label.assign(blk.label.begin() + r0, blk.label.begin() + r1);
    if (blk.weight.empty()) part_.weight.clear();
    else part_.weight.assign(blk.weight.begin() + r0, blk.weight.begin() + r1);
    part_.inherit_facts(blk);  // (a split block keeps its facts)
    fn(part_, r0);
    r0 = r1;
  }
}

double FtrlModel::train_block(const CsrBlock &blk, float *logit_out) {
  double total = 0.0;
  for_each_fitting(blk, [&](const CsrBlock &b, int r0) {
    double loss_sum = 0.0;
    const float *w = b.weight.empty() ? nullptr : b.weight.data();  // (null: the unweighted call)
    const Wire a = wire(b, grp_ != nullptr);  // (a group stages every block)
    if (grp_)
      check(ffm_group_train_batch_weighted(grp_, b.n_rows(), b.row_ptr.data(), a.field, b.feat.data(),
                                           a.val, b.label.data(), w, logit_out ? logit_out + r0 : nullptr, &loss_sum),
            "ffm_group_train_batch"), handed_over_++;  // (a group stages every block: its ordinal counts)
    else
      check(ffm_engine_train_batch_weighted(eng_, b.n_rows(), b.row_ptr.data(), a.field, b.feat.data(),
                                            a.val, b.label.data(), w, logit_out ? logit_out + r0 : nullptr,
                                            &loss_sum),
            "ffm_engine_train_batch");
    total += loss_sum;
  });
  return total;
}

void FtrlModel::train_block_async(const CsrBlock &blk) {
  for_each_fitting(blk, [&](const CsrBlock &b, int) {
    const float *w = b.weight.empty() ? nullptr : b.weight.data();  // (null: the unweighted call)
    const Wire a = wire(b, true);
    if (grp_)
      check(ffm_group_train_batch_async_weighted(grp_, b.n_rows(), b.row_ptr.data(), a.field, b.feat.data(),
                                                 a.val, b.label.data(), w, 0),
            "ffm_group_train_batch_async");
    else
      check(ffm_engine_train_batch_async_weighted(eng_, b.n_rows(), b.row_ptr.data(), a.field,
                                                  b.feat.data(), a.val, b.label.data(), w, 0),
            "ffm_engine_train_batch_async");
    handed_over_++;
  });
}

bool FtrlModel::pin_block(CsrBlock &blk, bool with_weights) {
  blk.row_ptr.reserve(static_cast<size_t>(max_rows_) + 1);
  blk.label.reserve(static_cast<size_t>(max_rows_));
  blk.field.reserve(static_cast<size_t>(max_nnz_));
  blk.feat.reserve(static_cast<size_t>(max_nnz_));
  blk.val.reserve(static_cast<size_t>(max_nnz_));
  void *ptr[5] = {blk.row_ptr.data(), blk.label.data(), blk.field.data(), blk.feat.data(), blk.val.data()};
  auto pages = [](size_t n) { return (4 * n + 4095) & ~static_cast<size_t>(4095); };  // (PageAllocator's)
  const size_t bytes[5] = {pages(blk.row_ptr.capacity()), pages(blk.label.capacity()), pages(blk.field.capacity()),
                           pages(blk.feat.capacity()), pages(blk.val.capacity())};
  for (int i = 0; i < 5; i++)
    if (ffm_engine_pin_host(ptr[i], bytes[i]) != FFM_OK) {
      for (int j = 0; j < i; j++) ffm_engine_unpin_host(ptr[j]);
      return false;
    }
  if (with_weights) {
    blk.weight.reserve(static_cast<size_t>(max_rows_));
    if (ffm_engine_pin_host(blk.weight.data(), pages(blk.weight.capacity())) != FFM_OK) {
      for (void *p : ptr) ffm_engine_unpin_host(p);
      return false;
    }
  }
  return true;
}

void FtrlModel::unpin_block(CsrBlock &blk) {
  void *ptr[5] = {blk.row_ptr.data(), blk.label.data(), blk.field.data(), blk.feat.data(), blk.val.data()};
  for (void *p : ptr) ffm_engine_unpin_host(p);
  if (blk.weight.capacity() > 0) ffm_engine_unpin_host(blk.weight.data());  // (pinned with the block: pin_block)
}

long long FtrlModel::train_block_pinned(const CsrBlock &blk) {
  const int n = blk.n_rows();
  bool fits = n <= max_rows_ && blk.row_ptr[n] <= max_nnz_;
  for (int r = 0; r < n && fits; r++) fits = blk.row_ptr[r + 1] - blk.row_ptr[r] <= max_row_nnz_;
  if (!fits) {  // (split into several calls, each copied: its arrays are free again on return)
    train_block_async(blk);
    return handed_over_;
  }
  const float *w = blk.weight.empty() ? nullptr : blk.weight.data();  // (null: the unweighted call)
  const Wire a = wire(blk, true);
  if (grp_)
    check(ffm_group_train_batch_async_weighted(grp_, n, blk.row_ptr.data(), a.field, blk.feat.data(),
                                               a.val, blk.label.data(), w, 1),
          "ffm_group_train_batch_async");
  else
    check(ffm_engine_train_batch_async_weighted(eng_, n, blk.row_ptr.data(), a.field, blk.feat.data(),
                                                a.val, blk.label.data(), w, 1),
          "ffm_engine_train_batch_async_pinned");
  return ++handed_over_;
}

long long FtrlModel::blocks_pulled() { return grp_ ? ffm_group_blocks_pulled(grp_) : ffm_engine_blocks_pulled(eng_); }

double FtrlModel::train_flush() {
  double loss_sum = 0.0;
  if (grp_) check(ffm_group_train_flush(grp_, &loss_sum), "ffm_group_train_flush");
  else check(ffm_engine_train_flush(eng_, &loss_sum), "ffm_engine_train_flush");
  return loss_sum;
}

void FtrlModel::enable_metrics(bool eval, bool train) {
  const int mask = (eval ? 1 << FFM_METRIC_EVAL : 0) | (train ? 1 << FFM_METRIC_TRAIN : 0);
  if (grp_) check(ffm_group_metrics_enable(grp_, mask), "ffm_group_metrics_enable");
  else check(ffm_engine_metrics_enable(eng_, mask), "ffm_engine_metrics_enable");
  metrics_mask_ = mask;
  if (keyed_field_ >= 0) enable_keyed_metrics(keyed_field_, keyed_rows_, eval, train);
}

void FtrlModel::enable_keyed_metrics(int field, long long capacity_rows, bool eval, bool train) {
  if (grp_) throw std::invalid_argument("keyed metrics: one GPU only");
  const int mask = (eval ? 1 << FFM_METRIC_EVAL : 0) | (train ? 1 << FFM_METRIC_TRAIN : 0);
  check(ffm_engine_metrics_key_field(eng_, mask, field, capacity_rows), "ffm_engine_metrics_key_field");
  keyed_mask_ = mask;
}

ffm_keyed_metrics FtrlModel::read_keyed_metrics(int channel, bool reset) {
  ffm_keyed_metrics m{};
  if (grp_) throw std::invalid_argument("keyed metrics: one GPU only");
  check(ffm_engine_metrics_read_keyed(eng_, channel, reset ? 1 : 0, &m), "ffm_engine_metrics_read_keyed");
  return m;
}

ffm_metrics FtrlModel::read_metrics(int channel, bool reset) {
  ffm_metrics m{};
  if (grp_) check(ffm_group_metrics_read(grp_, channel, reset ? 1 : 0, &m), "ffm_group_metrics_read");
  else check(ffm_engine_metrics_read(eng_, channel, reset ? 1 : 0, &m), "ffm_engine_metrics_read");
  return m;
}

ffm_refresh_stats FtrlModel::refresh_weights() {
  ffm_refresh_stats st{};
  if (grp_) check(ffm_group_refresh_weights(grp_, &st), "ffm_group_refresh_weights");
  else check(ffm_engine_refresh_weights(eng_, &st), "ffm_engine_refresh_weights");
  pull_linear();
  vec_w.dense_ready_ = false;
  vec_w.dense_.clear();
  vec_w.cache_.clear();
  return st;
}

// What differs between the two kinds of ablation: the noun of the messages and the engine's entry points.
static std::string ablation_noun(FtrlModel::Ablation kind) { return kind == FtrlModel::Ablation::Pairs ? "pair ablation" : "field ablation"; }

size_t FtrlModel::ablation_variants(Ablation kind) const {
  if (kind == Ablation::Fields) return static_cast<size_t>(n_fields) + 1;
  const int32_t pairs = ffm_engine_pair_count(n_fields);
  if (pairs < 0) throw std::invalid_argument("pair ablation: at most 64 fields");
  return static_cast<size_t>(pairs) + 1;
}

void FtrlModel::enable_ablation(Ablation kind, bool with_auc) {
  if (grp_) throw std::invalid_argument(ablation_noun(kind) + ": one GPU only");
  if (kind == Ablation::Pairs) check(ffm_engine_pair_ablation_enable(eng_, with_auc ? 1 : 0), "ffm_engine_pair_ablation_enable");
  else check(ffm_engine_ablation_enable(eng_, with_auc ? 1 : 0), "ffm_engine_ablation_enable");
}

void FtrlModel::set_pair_mask(const std::vector<uint64_t> &keep) {
  if (grp_) throw std::invalid_argument("a pair mask: one GPU only");
  const int rc = ffm_engine_set_pair_mask(eng_, keep.data(), static_cast<int32_t>(keep.size()));
  if (rc == FFM_E_INVALID || rc == FFM_E_UNSUPPORTED) throw std::invalid_argument(std::string("pair mask: ") + ffm_engine_last_error());
  check(rc, "ffm_engine_set_pair_mask");
}

void FtrlModel::predict_ablated_block(Ablation kind, const CsrBlock &blk, std::vector<double> &loss_sums) {
  if (grp_) throw std::invalid_argument(ablation_noun(kind) + ": one GPU only");
  const bool pairs = kind == Ablation::Pairs;
  const size_t variants = ablation_variants(kind);
  if (loss_sums.size() != variants)
    throw std::invalid_argument(ablation_noun(kind) + ": loss_sums needs " + (pairs ? "n_fields (n_fields + 1) / 2 + 1" : "n_fields + 1") + " entries");
  std::vector<double> part(variants);
  for_each_fitting(blk, [&](const CsrBlock &b, int) {
    check((pairs ? ffm_engine_predict_pair_ablated : ffm_engine_predict_ablated)(eng_, b.n_rows(), b.row_ptr.data(), b.field.data(), b.feat.data(),
                                                                                 b.val.data(), b.label.data(), 0, nullptr, part.data()),
          pairs ? "ffm_engine_predict_pair_ablated" : "ffm_engine_predict_ablated");
    for (size_t v = 0; v < variants; v++) loss_sums[v] += part[v];
  });
}

std::vector<ffm_metrics> FtrlModel::read_ablation_metrics(Ablation kind, bool reset) {
  if (grp_) throw std::invalid_argument(ablation_noun(kind) + ": one GPU only");
  std::vector<ffm_metrics> m(ablation_variants(kind));
  if (kind == Ablation::Pairs) check(ffm_engine_pair_ablation_read(eng_, reset ? 1 : 0, m.data()), "ffm_engine_pair_ablation_read");
  else check(ffm_engine_ablation_read(eng_, reset ? 1 : 0, m.data()), "ffm_engine_ablation_read");
  return m;
}

void FtrlModel::enable_pair_curve(const std::vector<uint16_t> &level, const std::vector<int32_t> &cuts, bool with_auc) {
  if (grp_) throw std::invalid_argument("the pruning curve: one GPU only");
  if (level.size() != static_cast<size_t>(n_fields) * static_cast<size_t>(n_fields))
    throw std::invalid_argument("the pruning curve: level needs n_fields * n_fields entries");
  const int rc = ffm_engine_pair_curve_enable(eng_, level.data(), n_fields, cuts.data(), static_cast<int32_t>(cuts.size()), with_auc ? 1 : 0);
  if (rc == FFM_E_INVALID || rc == FFM_E_UNSUPPORTED) throw std::invalid_argument(std::string("pair curve: ") + ffm_engine_last_error());
  check(rc, "ffm_engine_pair_curve_enable");
  curve_variants_ = cuts.size() + 1;
}

void FtrlModel::predict_curve_block(const CsrBlock &blk, std::vector<double> &loss_sums) {
  if (grp_) throw std::invalid_argument("the pruning curve: one GPU only");
  if (curve_variants_ == 0 || loss_sums.size() != curve_variants_)
    throw std::invalid_argument("the pruning curve: loss_sums needs one entry per cut and one for the rows (enable_pair_curve first)");
  std::vector<double> part(curve_variants_);
  for_each_fitting(blk, [&](const CsrBlock &b, int) {
    check(ffm_engine_predict_pair_curve(eng_, b.n_rows(), b.row_ptr.data(), b.field.data(), b.feat.data(), b.val.data(), b.label.data(), 0,
                                        nullptr, part.data()),
          "ffm_engine_predict_pair_curve");
    for (size_t v = 0; v < curve_variants_; v++) loss_sums[v] += part[v];
  });
}

std::vector<ffm_metrics> FtrlModel::read_curve_metrics(bool reset) {
  if (grp_) throw std::invalid_argument("the pruning curve: one GPU only");
  std::vector<ffm_metrics> m(std::max<size_t>(1, curve_variants_));
  check(ffm_engine_pair_curve_read(eng_, reset ? 1 : 0, m.data()), "ffm_engine_pair_curve_read");
  return m;
}

long long FtrlModel::predict_block_async(const CsrBlock &blk, bool pinned, float *scores, bool output_prob, bool *complete) {
  const int n = blk.n_rows();
  bool fits = n <= max_rows_ && blk.row_ptr[n] <= max_nnz_;
  for (int r = 0; r < n && fits; r++) fits = blk.row_ptr[r + 1] - blk.row_ptr[r] <= max_row_nnz_;
  bool device_writes = scores == nullptr;  // (nothing to write: the pipelined call as it always was)
  for (const auto &range : pinned_scores_)
    device_writes = device_writes || (scores >= range.first && scores + n <= range.first + range.second);
  if (complete) *complete = grp_ || !fits || !device_writes;
  if (grp_ || !fits || !device_writes) {  // a group predicts block by block (every shard, then the sum); so do split blocks
    eval_loss_pending_ += predict_block(blk, scores && output_prob, scores);
    return handed_over_;
  }
  const Wire a = wire(blk, true);
  if (scores)
    check(ffm_engine_predict_batch_async_scores(eng_, n, blk.row_ptr.data(), a.field, blk.feat.data(),
                                                a.val, blk.label.data(), pinned ? 1 : 0, output_prob ? 1 : 0, scores),
          "ffm_engine_predict_batch_async_scores");
  else
    check(ffm_engine_predict_batch_async(eng_, n, blk.row_ptr.data(), a.field, blk.feat.data(),
                                         a.val, blk.label.data(), pinned ? 1 : 0),
          "ffm_engine_predict_batch_async");
  return ++handed_over_;
}

void FtrlModel::check_resident(const ffm_rows_block &blk) const {
  if (grp_) throw std::invalid_argument("resident rows: one GPU only");
  if (blk.longest_row > max_row_nnz_)
    throw std::length_error("a row has " + std::to_string(blk.longest_row) + " entries; this engine handles up to " + std::to_string(max_row_nnz_));
}

long long FtrlModel::stage_block_resident(ffm_rows_block &blk) {
  check_resident(blk);
  check(ffm_engine_stage_batch_resident(eng_, &blk), "ffm_engine_stage_batch_resident");
  return ++handed_over_;
}

long long FtrlModel::train_block_resident(ffm_rows_block &blk) {
  check_resident(blk);
  check(ffm_engine_train_batch_async_resident(eng_, &blk), "ffm_engine_train_batch_async_resident");
  return ++handed_over_;
}

long long FtrlModel::predict_block_resident(ffm_rows_block &blk, float *scores, bool output_prob) {
  check_resident(blk);
  check(ffm_engine_predict_batch_async_resident(eng_, &blk, output_prob ? 1 : 0, scores), "ffm_engine_predict_batch_async_resident");
  return ++handed_over_;
}

long long FtrlModel::blocks_scored() { return grp_ ? 0 : ffm_engine_blocks_scored(eng_); }

bool FtrlModel::pin_scores(float *p, size_t n) {
  if (!p || !n || ffm_engine_pin_host(p, (4 * n + 4095) & ~static_cast<size_t>(4095)) != FFM_OK) return false;
  pinned_scores_.emplace_back(p, n);
  return true;
}

void FtrlModel::unpin_scores(float *p) {
  for (size_t i = 0; i < pinned_scores_.size(); i++)
    if (pinned_scores_[i].first == p) {
      ffm_engine_unpin_host(p);
      pinned_scores_.erase(pinned_scores_.begin() + static_cast<long>(i));
      return;
    }
}

double FtrlModel::eval_flush() {
  double loss_sum = 0.0;
  if (!grp_) check(ffm_engine_train_flush(eng_, &loss_sum), "ffm_engine_train_flush");
  loss_sum += eval_loss_pending_;
  eval_loss_pending_ = 0.0;
  return loss_sum;
}

double FtrlModel::predict_block(const CsrBlock &blk, bool output_prob, float *out) {
  double total = 0.0;
  for_each_fitting(blk, [&](const CsrBlock &b, int r0) {
    double loss_sum = 0.0;
    const Wire a = wire(b, false);
    if (grp_)
      check(ffm_group_predict_batch(grp_, b.n_rows(), b.row_ptr.data(), a.field, b.feat.data(),
                                    a.val, b.label.data(), output_prob ? 1 : 0,
                                    out ? out + r0 : nullptr, &loss_sum),
            "ffm_group_predict_batch");
    else
      check(ffm_engine_predict_batch(eng_, b.n_rows(), b.row_ptr.data(), a.field,
                                     b.feat.data(), a.val, b.label.data(), output_prob ? 1 : 0,
                                     out ? out + r0 : nullptr, &loss_sum),
            "ffm_engine_predict_batch");
    total += loss_sum;
  });
  return total;
}

// ---- the lazy latent mirror --------------------------------------------------------------------

size_t FtrlModel::stream_chunk() const {  // ~64 MB of floats per component and chunk
  const size_t per = static_cast<size_t>(std::max<int64_t>(row_len_, 1));
  return std::max<size_t>(1, std::min<size_t>(static_cast<size_t>(n_feats), (16u << 20) / per));
}

void FtrlModel::get_latent_rows(int component, size_t first, size_t count, float *out) {
  std::vector<int32_t> ids(count);
  for (size_t j = 0; j < count; j++) ids[j] = static_cast<int32_t>(first + j);
  std::vector<float> part;
  for (int r = 0; r < n_gpus_; r++) {
    float *dst = out;
    if (r > 0) {  // a shard stores only the slots it owns; the others read as 0: the model is the sum
      part.resize(count * static_cast<size_t>(row_len_));
      dst = part.data();
    }
    check(ffm_engine_get_rows(shard(r), static_cast<int32_t>(count), ids.data(), nullptr, nullptr, nullptr,
                              component == 0 ? dst : nullptr, component == 1 ? dst : nullptr,
                              component == 2 ? dst : nullptr),
          "ffm_engine_get_rows");
    if (r > 0)
      for (size_t i = 0; i < part.size(); i++) out[i] += part[i];
  }
}
void FtrlModel::set_latent_rows(int component, size_t first, size_t count, const float *in) {
  std::vector<int32_t> ids(count);
  for (size_t j = 0; j < count; j++) ids[j] = static_cast<int32_t>(first + j);
  for (int r = 0; r < n_gpus_; r++)  // (every shard keeps what it owns of them)
    check(ffm_engine_set_rows(shard(r), static_cast<int32_t>(count), ids.data(), nullptr, nullptr, nullptr,
                              component == 0 ? in : nullptr, component == 1 ? in : nullptr,
                              component == 2 ? in : nullptr),
          "ffm_engine_set_rows");
}

LatentMirror::row &LatentMirror::operator[](size_t i) {
  if (dense_ready_) return dense_[i];
  auto it = cache_.find(i);
  if (it != cache_.end()) return it->second;
  row r(row_len_);
  owner_->get_latent_rows(0, i, 1, r.data());
  return cache_.emplace(i, std::move(r)).first->second;
}
LatentMirror::row &LatentMirror::at(size_t i) {
  if (i >= n_) throw std::out_of_range("vec_w");
  return (*this)[i];
}
void LatentMirror::pull_all() {
  if (dense_ready_) return;
  dense_.assign(n_, row(row_len_));
  const size_t chunk = owner_->stream_chunk();
  std::vector<float> buf(chunk * row_len_);
  for (size_t f0 = 0; f0 < n_; f0 += chunk) {
    const size_t nf = std::min(chunk, n_ - f0);
    owner_->get_latent_rows(0, f0, nf, buf.data());
    for (size_t j = 0; j < nf; j++) std::copy(buf.begin() + j * row_len_, buf.begin() + (j + 1) * row_len_, dense_[f0 + j].begin());
  }
  for (auto &kv : cache_) dense_[kv.first] = std::move(kv.second);  // (rows edited before the pull win)
  cache_.clear();
  dense_ready_ = true;
}

void FtrlModel::pull_weights() {
  pull_linear();
  if (vec_w.dense_ready_) {
    vec_w.dense_ready_ = false;
    vec_w.cache_.clear();
    vec_w.pull_all();
  } else {
    for (auto &kv : vec_w.cache_) get_latent_rows(0, kv.first, 1, kv.second.data());
  }
}

void FtrlModel::push_weights() {
  push_linear();
  if (vec_w.dense_ready_) {
    const size_t chunk = stream_chunk(), rl = static_cast<size_t>(row_len_);
    std::vector<float> buf(chunk * rl);
    for (size_t f0 = 0; f0 < vec_w.n_; f0 += chunk) {
      const size_t nf = std::min(chunk, vec_w.n_ - f0);
      for (size_t j = 0; j < nf; j++) std::copy(vec_w.dense_[f0 + j].begin(), vec_w.dense_[f0 + j].end(), buf.begin() + j * rl);
      set_latent_rows(0, f0, nf, buf.data());
    }
  } else {
    for (auto &kv : vec_w.cache_) set_latent_rows(0, kv.first, 1, kv.second.data());
  }
}

// ---- model files, streamed (persist.h) -----------------------------------------------------------

void FtrlModel::save_model(std::string_view file_name) {  // ffm.cpp:163-180
  pull_linear();
  TextModelWriter w{std::string(file_name)};
  w.scalar(bias);
  for (float v : lin_w) w.scalar(v);
  const size_t chunk = stream_chunk(), rl = static_cast<size_t>(row_len_), nf = rl ? static_cast<size_t>(n_feats) : 0;
  std::vector<float> buf(chunk * rl);
  for (size_t f0 = 0; f0 < nf; f0 += chunk) {
    const size_t n = std::min(chunk, nf - f0);
    get_latent_rows(0, f0, n, buf.data());
    w.rows(buf.data(), n, rl);
  }
  w.finish();
}
void FtrlModel::load_model(std::string_view file_name) {  // ffm.cpp:182-200
  TextModelReader r{std::string(file_name)};
  bias = r.scalar();
  for (auto &v : lin_w) v = r.scalar();
  push_linear();
  const size_t chunk = stream_chunk(), rl = static_cast<size_t>(row_len_), nf = rl ? static_cast<size_t>(n_feats) : 0;
  std::vector<float> buf(chunk * rl);
  for (size_t f0 = 0; f0 < nf; f0 += chunk) {
    const size_t n = std::min(chunk, nf - f0);
    r.rows(buf.data(), n, rl);
    set_latent_rows(0, f0, n, buf.data());
  }
  vec_w.dense_ready_ = false;
  vec_w.dense_.clear();
  vec_w.cache_.clear();
}
void FtrlModel::save_compressed_model(std::string_view file_name, int compress_level) {  // ffm.cpp:138-146
  pull_linear();
  const size_t rl = static_cast<size_t>(row_len_), nf = static_cast<size_t>(n_feats);
  FloatFrameWriter w(std::string(file_name), 1 + nf + nf * rl, compress_level);
  w.write(&bias, 1);
  w.write(lin_w.data(), nf);
  const size_t chunk = stream_chunk();
  std::vector<float> buf(chunk * rl);
  for (size_t f0 = 0; rl && f0 < nf; f0 += chunk) {
    const size_t n = std::min(chunk, nf - f0);
    get_latent_rows(0, f0, n, buf.data());
    w.write(buf.data(), n * rl);
  }
  w.finish();
}
void FtrlModel::load_compressed_model(std::string_view file_name) {  // ffm.cpp:148-161
  const size_t rl = static_cast<size_t>(row_len_), nf = static_cast<size_t>(n_feats);
  FloatFrameReader r{std::string(file_name)};
  if (r.total_floats() != 1 + nf + nf * rl) throw std::runtime_error(std::string(file_name) + ": holds a model of a different shape");
  auto need = [&](float *p, size_t n) {
    if (r.read(p, n) != n) throw std::runtime_error(std::string(file_name) + ": zstd frame is truncated");
  };
  need(&bias, 1);
  need(lin_w.data(), nf);
  push_linear();
  const size_t chunk = stream_chunk();
  std::vector<float> buf(chunk * rl);
  for (size_t f0 = 0; rl && f0 < nf; f0 += chunk) {
    const size_t n = std::min(chunk, nf - f0);
    need(buf.data(), n * rl);
    set_latent_rows(0, f0, n, buf.data());
  }
  std::printf("loading from %s, floats: %zu\n", std::string(file_name).c_str(), r.total_floats());
  vec_w.dense_ready_ = false;
  vec_w.dense_.clear();
  vec_w.cache_.clear();
}

// [bias_n, bias_z, lin_n[], lin_z[], vec_n[], vec_z[]], one zstd frame
void FtrlModel::save_state(std::string_view file_name, int compress_level) {
  const size_t nf = static_cast<size_t>(n_feats), rl = static_cast<size_t>(row_len_);
  FloatFrameWriter w(std::string(file_name), 2 + 2 * nf + 2 * nf * rl, compress_level);
  float b2[2];
  std::vector<float> lin(nf);
  // bias and linear accumulators from the shards that own them
  auto linear_state = [&](bool z_row) {
    std::vector<float> tmp(nf);
    for (int r = 0; r < n_gpus_; r++) {
      float bn = 0.0f, bz = 0.0f;
      check(ffm_engine_get_state(shard(r), &bn, &bz, z_row ? nullptr : tmp.data(), z_row ? tmp.data() : nullptr, nullptr, nullptr),
            "ffm_engine_get_state");
      if (r == bias_owner_ || !grp_) { b2[0] = bn; b2[1] = bz; }
      for (size_t i = 0; i < nf; i++)
        if (!grp_ || lin_owner_of_field_[field_of(static_cast<int>(i))] == r) lin[i] = tmp[i];
    }
  };
  linear_state(false);
  w.write(b2, 2);
  w.write(lin.data(), nf);
  linear_state(true);
  w.write(lin.data(), nf);
  const size_t chunk = stream_chunk();
  std::vector<float> buf(chunk * rl);
  for (int comp = 1; comp <= 2 && rl; comp++)
    for (size_t f0 = 0; f0 < nf; f0 += chunk) {
      const size_t n = std::min(chunk, nf - f0);
      get_latent_rows(comp, f0, n, buf.data());
      w.write(buf.data(), n * rl);
    }
  w.finish();
}
void FtrlModel::load_state(std::string_view file_name) {
  const size_t nf = static_cast<size_t>(n_feats), rl = static_cast<size_t>(row_len_);
  FloatFrameReader r{std::string(file_name)};
  if (r.total_floats() != 2 + 2 * nf + 2 * nf * rl) throw std::runtime_error(std::string(file_name) + ": wrong shape");
  auto need = [&](float *p, size_t n) {
    if (r.read(p, n) != n) throw std::runtime_error(std::string(file_name) + ": zstd frame is truncated");
  };
  float b2[2];
  std::vector<float> lin(nf);
  need(b2, 2);
  need(lin.data(), nf);
  for (int r = 0; r < n_gpus_; r++)
    check(ffm_engine_set_state(shard(r), &b2[0], &b2[1], lin.data(), nullptr, nullptr, nullptr), "ffm_engine_set_state");
  need(lin.data(), nf);
  for (int r = 0; r < n_gpus_; r++)
    check(ffm_engine_set_state(shard(r), nullptr, nullptr, nullptr, lin.data(), nullptr, nullptr), "ffm_engine_set_state");
  const size_t chunk = stream_chunk();
  std::vector<float> buf(chunk * rl);
  for (int comp = 1; comp <= 2 && rl; comp++)
    for (size_t f0 = 0; f0 < nf; f0 += chunk) {
      const size_t n = std::min(chunk, nf - f0);
      need(buf.data(), n * rl);
      set_latent_rows(comp, f0, n, buf.data());
    }
}

// ---- sparse checkpoint: the records that differ from a freshly constructed model ------------------

static uint32_t float_bits(float v) {
  uint32_t b;
  std::memcpy(&b, &v, sizeof b);
  return b;
}

void FtrlModel::save_checkpoint(std::string_view file_name, int compress_level, TrainProgress progress) {
  if (n_gpus_ > 1) throw std::runtime_error("sparse checkpoints are not supported for sharded models (--n_gpus > 1)");
  const size_t rl = static_cast<size_t>(row_len_);
  // one scan; the id buffer is sized for every feature and only the pages written are ever committed
  std::unique_ptr<int32_t[]> ids(new int32_t[static_cast<size_t>(n_feats)]);
  int64_t n = 0;
  check(ffm_engine_changed_features(eng_, ids.get(), n_feats, &n), "ffm_engine_changed_features");
  SparseCheckpointHeader h;
  h.model_type = static_cast<int32_t>(model_type);
  h.n_feats = n_feats;
  h.n_fields = n_fields;
  h.n_factors = n_factors;
  h.flags = static_cast<uint32_t>(flags_);
  h.row_len = row_len_;
  h.seed = seed_;
  h.init_mean_bits = float_bits(init_mean_);
  h.init_stddev_bits = float_bits(init_stddev_);
  h.n_changed = n;
  h.chunk = static_cast<int64_t>(stream_chunk());
  float b3[3] = {0.0f, 0.0f, 0.0f};
  check(ffm_engine_get_weights(eng_, &b3[0], nullptr, nullptr), "ffm_engine_get_weights");
  check(ffm_engine_get_state(eng_, &b3[1], &b3[2], nullptr, nullptr, nullptr, nullptr), "ffm_engine_get_state");
  for (int i = 0; i < 3; i++) h.bias_bits[i] = float_bits(b3[i]);
  h.rows_seen = progress.rows_seen;
  h.epochs_done = progress.epochs_done;
  SparseCheckpointWriter w(std::string(file_name), h, ids.get(), compress_level);
  const size_t chunk = std::min(static_cast<size_t>(h.chunk), static_cast<size_t>(std::max<int64_t>(n, 1)));
  std::vector<float> lin(3 * chunk), vec(3 * chunk * rl);
  for (size_t j0 = 0; j0 < static_cast<size_t>(n); j0 += chunk) {
    const size_t c = std::min(chunk, static_cast<size_t>(n) - j0);
    float *lw = lin.data(), *ln = lw + c, *lz = ln + c;
    float *vw = rl ? vec.data() : nullptr, *vn = rl ? vw + c * rl : nullptr, *vz = rl ? vn + c * rl : nullptr;
    check(ffm_engine_get_rows(eng_, static_cast<int32_t>(c), ids.get() + j0, lw, ln, lz, vw, vn, vz), "ffm_engine_get_rows");
    w.chunk(c, lw, ln, lz, vw, vn, vz);
  }
  w.finish();
}

FtrlModel::TrainProgress FtrlModel::load_checkpoint(std::string_view file_name) {
  if (n_gpus_ > 1) throw std::runtime_error("sparse checkpoints are not supported for sharded models (--n_gpus > 1)");
  const std::string name(file_name);
  SparseCheckpointReader r(name);
  const SparseCheckpointHeader &h = r.header();
  if (h.model_type != static_cast<int32_t>(model_type) || h.n_feats != n_feats || h.row_len != row_len_ ||
      (row_len_ > 0 && h.n_factors != n_factors) || (model_type == ModelType::FFM && h.n_fields != n_fields))
    throw std::runtime_error(name + ": holds a model of a different shape");
  if (h.seed != seed_ || h.init_mean_bits != float_bits(init_mean_) || h.init_stddev_bits != float_bits(init_stddev_) ||
      ((h.flags ^ static_cast<uint32_t>(flags_)) & FFM_FLAG_SKIP_INIT))
    throw std::runtime_error(name + ": was saved from a model with another seed or other init parameters "
                                    "(its records are deltas to THAT fresh model)");
  if ((h.flags ^ static_cast<uint32_t>(flags_)) & FFM_FLAG_LEARN)
    throw std::runtime_error(name + ": was saved " + ((h.flags & FFM_FLAG_LEARN) ? "with" : "without") +
                             " --learn, this model is the other variant: the resumed run would not be the interrupted one");
  if ((h.flags ^ static_cast<uint32_t>(flags_)) & FFM_FLAG_HASH_IDS)
    throw std::runtime_error(name + ": was saved " + ((h.flags & FFM_FLAG_HASH_IDS) ? "with" : "without") +
                             " --hash_feats, this model is the other variant: the resumed run would not be the interrupted one");
  if ((h.flags ^ static_cast<uint32_t>(flags_)) & FFM_FLAG_NORM_ROWS)
    throw std::runtime_error(name + ": was saved " + ((h.flags & FFM_FLAG_NORM_ROWS) ? "with" : "without") +
                             " --normalize_rows, this model is the other variant: the resumed run would not be the interrupted one");
  int64_t touched = 0;
  // (a serving model is built and loaded once by the CLI; it has no scan to prove that it is fresh)
  if (!serving_) check(ffm_engine_changed_features(eng_, nullptr, 0, &touched), "ffm_engine_changed_features");
  if (touched != 0)
    throw std::runtime_error(name + ": a sparse checkpoint loads into a fresh model only; " + std::to_string(touched) +
                             " features of this one have changed already");
  float b3[3];
  for (int i = 0; i < 3; i++) std::memcpy(&b3[i], &h.bias_bits[i], sizeof(float));
  check(ffm_engine_set_weights(eng_, &b3[0], nullptr, nullptr), "ffm_engine_set_weights");
  if (!serving_) check(ffm_engine_set_state(eng_, &b3[1], &b3[2], nullptr, nullptr, nullptr, nullptr), "ffm_engine_set_state");
  const size_t rl = static_cast<size_t>(row_len_), n = r.ids().size();
  const size_t cap = std::min(static_cast<size_t>(h.chunk), std::max<size_t>(n, 1));
  std::vector<float> lin(3 * cap), vec(3 * cap * rl);
  size_t j0 = 0;
  while (const size_t c = r.next_chunk_size()) {
    float *lw = lin.data(), *ln = lw + c, *lz = ln + c;
    float *vw = rl ? vec.data() : nullptr, *vn = rl ? vw + c * rl : nullptr, *vz = rl ? vn + c * rl : nullptr;
    r.chunk(lw, ln, lz, vw, vn, vz);
    if (serving_)  // only the ids, lin_w and vec_w (rounded to the engine's format on the device)
      check(ffm_engine_set_rows(eng_, static_cast<int32_t>(c), r.ids().data() + j0, lw, nullptr, nullptr, vw, nullptr, nullptr), "ffm_engine_set_rows");
    else
    check(ffm_engine_set_rows(eng_, static_cast<int32_t>(c), r.ids().data() + j0, lw, ln, lz, vw, vn, vz), "ffm_engine_set_rows");
    j0 += c;
  }
  r.finish();
  std::printf("loading from %s, changed features: %zu of %d\n", name.c_str(), n, n_feats);
  pull_linear();
  vec_w.dense_ready_ = false;
  vec_w.dense_.clear();
  vec_w.cache_.clear();
  TrainProgress p;
  p.rows_seen = h.rows_seen;
  p.epochs_done = h.epochs_done;
  return p;
}

// ---- serving deltas: what a shadow serving engine had to move to follow this model -----------------

void FtrlModel::make_shadow(const std::string &fmt) {
  if (shadow_) {
    if (fmt != shadow_fmt_) throw std::invalid_argument("publish_delta: the shadow is " + shadow_fmt_ + ", not " + fmt);
    return;
  }
  if (fmt != "f32" && fmt != "f16") throw std::invalid_argument("publish_delta: the format is f32 or f16");
  if (serving_ || grp_ || n_gpus_ > 1 || model_type != ModelType::FFM)
    throw std::invalid_argument("publish_delta follows one whole FFM training engine on one GPU");
  // a serving engine of this model's shape, seed and init: fresh, it is what a consumer starts from
  ffm_engine_config cfg;
  ffm_engine_default_config(&cfg);
  cfg.model_type = FFM_MODEL_FFM;
  cfg.n_feats = n_feats;
  cfg.n_fields = n_fields;
  cfg.n_factors = n_factors;
  cfg.init_mean = init_mean_;
  cfg.init_stddev = init_stddev_;
  cfg.seed = seed_;
  cfg.max_batch_rows = 1;  // (it never predicts)
  cfg.max_batch_nnz = 128;
  cfg.max_row_nnz = 128;
  cfg.device_id = device_;
  cfg.flags = (flags_ & FFM_FLAG_SKIP_INIT) | (fmt == "f16" ? FFM_FLAG_SERVE_F16 : FFM_FLAG_SERVE_F32);
  const int rc = ffm_engine_create(&cfg, &shadow_);
  if (rc == FFM_E_INVALID || rc == FFM_E_UNSUPPORTED) throw std::invalid_argument(ffm_engine_last_error());
  check(rc, "ffm_engine_create (the publishing shadow)");
  shadow_fmt_ = fmt;
  shadow_seq_ = 0;
}

void FtrlModel::prepare_publish(const std::string &prefix, const std::string &fmt, long long seq_done) {
  make_shadow(fmt);
  while (shadow_seq_ < seq_done) {
    apply_delta_to(shadow_, shadow_fmt_, prefix + "." + std::to_string(shadow_seq_ + 1) + ".delta", shadow_seq_ + 1);
    shadow_seq_++;
  }
}

static long long file_bytes(const std::string &path) {
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  return f.good() ? static_cast<long long>(f.tellg()) : 0;
}

FtrlModel::DeltaResult FtrlModel::publish_delta(const std::string &prefix, const std::string &fmt, long long seq) {
  make_shadow(fmt);
  if (seq != shadow_seq_ + 1)
    throw std::runtime_error("publish_delta: delta " + std::to_string(seq) + " asked for, the shadow has " +
                             std::to_string(shadow_seq_) + " behind it");
  ffm_sync_stats st;
  check(ffm_engine_sync_weights(shadow_, eng_, &st), "ffm_engine_sync_weights");
  int64_t n = 0;
  check(ffm_engine_sync_moved(shadow_, nullptr, 0, &n), "ffm_engine_sync_moved");
  std::vector<int32_t> ids(static_cast<size_t>(std::max<int64_t>(n, 1)));
  check(ffm_engine_sync_moved(shadow_, ids.data(), n, &n), "ffm_engine_sync_moved");
  ServeDeltaHeader h;
  h.model_type = static_cast<int32_t>(model_type);
  h.n_feats = n_feats;
  h.n_fields = n_fields;
  h.n_factors = n_factors;
  h.hash_ids = (flags_ & FFM_FLAG_HASH_IDS) ? 1u : 0u;
  h.format = fmt == "f16" ? kServeDeltaF16 : kServeDeltaF32;
  h.row_len = row_len_;
  h.seed = seed_;
  h.init_mean_bits = float_bits(init_mean_);
  h.init_stddev_bits = float_bits(init_stddev_);
  h.seq = seq;
  h.n_moved = n;
  h.chunk = static_cast<int64_t>(stream_chunk());
  float b = 0.0f;
  check(ffm_engine_get_weights(shadow_, &b, nullptr, nullptr), "ffm_engine_get_weights");
  h.bias_bits = float_bits(b);
  DeltaResult res;
  res.file = prefix + "." + std::to_string(seq) + ".delta";
  res.n_moved = n;
  ServeDeltaWriter w(res.file, h, ids.data(), 3);
  const size_t chunk = std::min(static_cast<size_t>(h.chunk), static_cast<size_t>(std::max<int64_t>(n, 1)));
  std::vector<float> lin(chunk), lat(chunk * h.row_words());
  for (size_t j0 = 0; j0 < static_cast<size_t>(n); j0 += chunk) {
    const size_t c = std::min(chunk, static_cast<size_t>(n) - j0);
    check(ffm_engine_get_rows_raw(shadow_, static_cast<int32_t>(c), ids.data() + j0, lin.data(), lat.data()), "ffm_engine_get_rows_raw");
    w.chunk(c, lin.data(), lat.data());
  }
  w.finish();
  shadow_seq_ = seq;
  res.bytes = file_bytes(res.file);
  return res;
}

FtrlModel::DeltaResult FtrlModel::apply_delta_to(ffm_engine *e, const std::string &fmt, const std::string &path, long long want_seq) {
  ServeDeltaReader r(path);
  const ServeDeltaHeader &h = r.header();
  if (h.model_type != static_cast<int32_t>(model_type) || h.n_feats != n_feats || h.n_fields != n_fields ||
      h.n_factors != n_factors || h.row_len != row_len_)
    throw std::runtime_error(path + ": holds the rows of a model of a different shape");
  if (h.format != (fmt == "f16" ? kServeDeltaF16 : kServeDeltaF32))
    throw std::runtime_error(path + ": holds " + (h.format == kServeDeltaF16 ? "f16" : "f32") + " rows, this serving engine is " + fmt);
  if (h.hash_ids != ((flags_ & FFM_FLAG_HASH_IDS) ? 1u : 0u))
    throw std::runtime_error(path + ": was published " + (h.hash_ids ? "with" : "without") + " --hash_feats, this model is the other variant");
  if (h.seed != seed_ || h.init_mean_bits != float_bits(init_mean_) || h.init_stddev_bits != float_bits(init_stddev_))
    throw std::runtime_error(path + ": was published from a model with another seed or other init parameters "
                                    "(delta 1 is relative to THAT fresh model)");
  if (h.seq != want_seq)
    throw std::runtime_error(path + ": is delta " + std::to_string(h.seq) + ", the next one to apply is " + std::to_string(want_seq));
  const size_t n = r.ids().size();
  const size_t cap = std::min(static_cast<size_t>(h.chunk), std::max<size_t>(n, 1));
  std::vector<float> lin(cap), lat(cap * h.row_words());
  size_t j0 = 0;
  while (const size_t c = r.next_chunk_size()) {
    r.chunk(lin.data(), lat.data());
    check(ffm_engine_set_rows_raw(e, static_cast<int32_t>(c), r.ids().data() + j0, lin.data(), lat.data()), "ffm_engine_set_rows_raw");
    j0 += c;
  }
  r.finish();
  float b;
  std::memcpy(&b, &h.bias_bits, sizeof b);
  check(ffm_engine_set_weights(e, &b, nullptr, nullptr), "ffm_engine_set_weights");
  DeltaResult res;
  res.file = path;
  res.n_moved = static_cast<long long>(n);
  res.bytes = file_bytes(path);
  return res;
}

FtrlModel::DeltaResult FtrlModel::apply_delta(const std::string &path) {
  if (!serving_) throw std::invalid_argument("apply_delta fills a serving model (--serve_weights f32 | f16)");
  const DeltaResult res = apply_delta_to(eng_, serve_fmt_, path, deltas_applied_ + 1);
  deltas_applied_++;
  pull_linear();
  vec_w.dense_ready_ = false;
  vec_w.dense_.clear();
  vec_w.cache_.clear();
  return res;
}

bool FtrlModel::has_zero_weights() {  // utils.h:63-76 over lin_w, then vec_w (ftrl_offline.cpp:105-119)
  pull_linear();
  if (std::any_of(lin_w.begin(), lin_w.end(), [](float w) { return w == 0.0f; })) return true;
  const size_t chunk = stream_chunk(), rl = static_cast<size_t>(row_len_), nf = rl ? static_cast<size_t>(n_feats) : 0;
  std::vector<float> buf(chunk * rl);
  for (size_t f0 = 0; f0 < nf; f0 += chunk) {  // streamed: stops at the first chunk that holds a zero
    const size_t n = std::min(chunk, nf - f0);
    get_latent_rows(0, f0, n, buf.data());
    if (std::any_of(buf.begin(), buf.begin() + n * rl, [](float w) { return w == 0.0f; })) return true;
  }
  return false;
}

std::unique_ptr<FtrlModel> make_model(const config_options &opt) {
  if (opt.model_type == "LR") return std::make_unique<LR>(opt);
  if (opt.model_type == "FM") return std::make_unique<FM>(opt);
  if (opt.model_type == "FFM") return std::make_unique<FFM>(opt);
  std::fprintf(stderr, "Invalid model_type: %s, expect `LR`, `FM` or `FFM`.\n", opt.model_type.c_str());
  throw std::invalid_argument("invalid model_type");
}

}  // namespace ftrl
