/*
 * ffm_engine.h -- C ABI of the MI355X (gfx950) FTRL LR/FM/FFM training engine.
 *
 * This is the drop-in boundary for ONE path of massquantity/Ftrl-FFM: the forward + gradient +
 * FTRL per-coordinate update behind ftrl::FtrlModel (reference src/include/model/ftrl_model.h:14-51)
 * as called by FtrlOffline::one_epoch (src/task/ftrl_offline.cpp:74-83), FtrlOnline::run_task
 * (src/task/ftrl_online.cpp:70-80) and Evaluator::run_task (src/eval/evaluate.cpp:23-33).
 * Plain pointers and sizes only; no C++ or torch types.  Every entry point returns 0 on success
 * and a negative FFM_E_* code on failure (message via ffm_engine_last_error()); nothing throws.
 * The library contains no CPU fallback: without a usable HIP device ffm_engine_create fails.
 *
 * Wire format of a block of rows ("batch"): CSR over (field, feat, val) entries --
 *   row_ptr[n_rows+1] int32, field[nnz] int32, feat[nnz] int32, val[nnz] float32, label[n_rows]
 *   int32 (0/1) -- i.e. the reference's Sample{feat_vec x; int y} (src/include/data/sample.h:6-9,
 *   src/include/utils/types.h:18-19) flattened.  field may be NULL for LR/FM (libsvm rows, field 0).
 *   The host-buffer entry points that upload through a staging slot (ffm_engine_stage_batch,
 *   ffm_engine_train_batch_async[_pinned], ffm_engine_predict_batch_async, and ffm_group_train_batch[_async],
 *   which stage through them) also take field == NULL
 *   for FFM: the block's rows must then hold exactly one entry per field, entry j of a row being
 *   field j's (what python/generate_data.py:272-306 writes and a libffm file without dropped zeros
 *   is; anything else is FFM_E_INVALID) -- the field array is then written on the device instead
 *   of crossing PCIe, a third of the block's bytes.  Same results as with the array passed.
 *   Every entry point that takes rows in HOST memory, the synchronous ones included, takes val == NULL: every
 *   value is 1.0f -- "Rows without values" below.
 *   Entries whose feat (FFM: or field) is out of range are ignored exactly as
 *   FtrlModel::remove_out_range / FFM::remove_out_range erase them (ftrl_model.cpp:36-42,
 *   ffm.cpp:30-36); the caller's buffers are never modified.  (FFM_FLAG_HASH_IDS: ids >= n_feats are
 *   hashed into range instead -- "Hashed ids" below.)
 *
 * Batch semantics: all rows of one train call see the weights refreshed from the
 * call-start (n,z); each touched (n,z) then receives the reference's per-sample update once per
 * touching (row, pair) in row order.  A call with n_rows == 1 is exactly one reference
 * FtrlModel::train().
 */
#ifndef FFM_ENGINE_H
#define FFM_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3: + ffm_engine_predict_batch_async, ffm_group_* (additions only: a caller built against 2 runs
 * unchanged).  The *_weighted entry points ("Sample weights" below) and ffm_engine_refresh_weights /
 * ffm_group_refresh_weights ("Refresh" below) are additions as well, and so are FFM_FLAG_HASH_IDS and
 * ffm_engine_hash_ids_device / _host ("Hashed ids" below). */
#define FFM_ENGINE_ABI_VERSION 4

/* ModelType, reference src/include/utils/types.h:21-25 */
enum { FFM_MODEL_LR = 0, FFM_MODEL_FM = 1, FFM_MODEL_FFM = 2 };

enum {
  FFM_OK = 0,
  FFM_E_INVALID = -1,   /* bad argument (std::invalid_argument in the reference) */
  FFM_E_DEVICE = -2,    /* HIP runtime error / no device */
  FFM_E_NOMEM = -3,     /* device allocation failed */
  FFM_E_CAPACITY = -4,  /* batch exceeds max_batch_rows / max_batch_nnz */
  FFM_E_UNSUPPORTED = -5
};

typedef struct ffm_engine ffm_engine;

/* Replaces config_options (reference src/include/utils/cmd_option.h:29-66) for this path; the
 * defaults written by ffm_engine_default_config are the reference's (:49-63). */
typedef struct ffm_engine_config {
  int32_t model_type;      /* FFM_MODEL_* ; opt.model_type */
  int32_t n_feats;         /* opt.n_feats   (10000) */
  int32_t n_fields;        /* opt.n_fields  (8); ignored for LR/FM */
  int32_t n_factors;       /* opt.n_factors (16); ignored for LR */
  float w_alpha;           /* 1e-4 */
  float w_beta;            /* 1.0 */
  float w_l1;              /* 0.1 */
  float w_l2;              /* 5.0 */
  float init_mean;         /* 0.0 */
  float init_stddev;       /* 0.02 */
  uint64_t seed;           /* the reference is unseeded (utils.h:30-36); here init is reproducible */
  int32_t max_batch_rows;  /* capacity of one train/predict call */
  int32_t max_batch_nnz;   /* capacity in entries of one call */
  int32_t device_id;       /* HIP device ordinal */
  /* Field-pair sharding of the latent tensor over the GPUs of a node (FFM; DESIGN.md
   * "Multi-GPU"): this engine owns both latent slots of the field pairs ffm_engine_shard_plan
   * assigns to shard_rank -- contiguous blocks of the field x field triangle -- and the bias /
   * linear terms that plan gives it. */
  int32_t n_shards;        /* 1 */
  int32_t shard_rank;      /* 0 */
  void *stream;            /* hipStream_t to run on; NULL = the engine creates its own */
  int32_t flags;           /* FFM_FLAG_* */
  int32_t max_row_nnz;     /* longest row a call may hold (LDS staging of the row kernels); 0 = 1024 (serving engines: 128) */
  /* Per-field id ranges: field f owns the ids [field_start[f], field_start[f+1]), n_fields + 1
   * ascending values from 0 to n_feats (python/generate_data.py:272-306 and the bundled data lay
   * ids out like this).  NULL = unknown.  With it a sharded engine stores only the records of the
   * fields it has pairs of, and in each record only the slots it owns -- about 1/n_shards of the
   * (n_feats x n_fields x n_factors) tensor -- and it skips the columns of the other fields; an
   * entry whose id is outside its field's range then voids its block (FFM_E_INVALID at the next
   * sync).  Without it every shard keeps full-length records and only the work is sharded.
   * With n_shards == 1 it is a HINT: the block grouping (the mini-batch scheduler that replaces the
   * per-feature mutexes of src/include/model/ffm.h:32) sorts every field's id range by itself in one
   * launch, and blocks whose rows are one entry per field in field order take shorter forms of the
   * update; ids that sit under another field than their range's are still handled correctly.  The
   * array is copied. */
  const int32_t *field_start;
  int32_t reserved[4];
} ffm_engine_config;

enum {
  FFM_FLAG_SKIP_INIT = 1, /* leave w zeroed; the caller will ffm_engine_set_weights */
  FFM_FLAG_LEARN = 4,     /* opt-in "learning" variant, NOT the reference's arithmetic (SURVEY.md
                           * 8(f) rank 4): (1) the lazy refresh keeps a latent slot's initial
                           * weight until its first gradient (n > 0) instead of overwriting it
                           * with W(0,0) = 0 (ffm.cpp:72-88, fm.cpp:69-78), (2) ffm.cpp:118 uses
                           * g2*g2 instead of g2*g1 -- so that FM / FFM factors actually train.
                           * Off: the reference bit for bit.  (Flag value 2 was round 1's
                           * optional fused row kernel: measured slower, removed.) */
  FFM_FLAG_HASH_IDS = 8,  /* feature ids of HOST rows are hashed into their field's id range on the device
                           * before any kernel reads them: "Hashed ids" below */
  FFM_FLAG_SERVE_F32 = 16, /* a SERVING engine: weights only, for prediction -- "Serving engines" below; */
  FFM_FLAG_SERVE_F16 = 32, /* its latent table in fp32 bits or in IEEE binary16 (both: FFM_E_INVALID) */
  FFM_FLAG_NORM_ROWS = 64  /* every HOST row is scaled to unit Euclidean length on the device before any kernel
                            * reads its values (libffm's and xLearn's instance-wise normalisation):
                            * "Normalised rows" below */
};

void ffm_engine_default_config(ffm_engine_config *cfg);

/* Replaces the FtrlModel / LR / FM / FFM constructors (ftrl_model.cpp:12-34, fm.cpp:9-19,
 * ffm.cpp:17-28): allocates bias, linear and latent (w,n,z) in HBM, zeroes n,z and draws w from
 * N(init_mean, init_stddev) with a counter-based generator keyed by cfg->seed. */
int ffm_engine_create(const ffm_engine_config *cfg, ffm_engine **out);
/* The initial weights ffm_engine_create draws, recomputed on the HOST (no device needed): element
 * j of out is lin_w[first + j] (latent == 0) or vec_w flattened [feat][row_len] at first + j
 * (latent != 0).  The generator is a pure function of (seed, array, index) evaluated with
 * correctly rounded operations only (csrc/init_rng.h), so these are the device's bits -- the
 * reference's initialiser (utils.h:30-61) is unseeded and cannot be reproduced at all. */
int ffm_engine_init_weights_host(uint64_t seed, float init_mean, float init_stddev, int32_t latent,
                                 int64_t first, int64_t count, float *out);
void ffm_engine_destroy(ffm_engine *e);
const char *ffm_engine_last_error(void);
int ffm_engine_abi_version(void);
/* Block-update semantics, part of the contract (INTEGRATION.md "Block semantics"): a call with
 * n_rows == 1 is the reference's train() bit for bit (src/model/ffm.cpp:38-49); a block of several
 * rows folds the touches of every (n, z) accumulator by reductions over segments of this many
 * consecutive occurrences of its feature, joined left to right (csrc/kernels_fold.h).  Two builds
 * that return different values here train bit-different models from the same blocks. */
int ffm_engine_block_segment(void);

/* The partition behind n_shards / shard_rank, as plain host arithmetic (no device needed): the
 * fields are cut into contiguous groups and every shard owns whole group x group blocks of field
 * pairs, so the partner fields a shard owns for any field form ONE contiguous range (2 shards: 2
 * groups; 4 and 8 shards: 4 groups -- at 8 a shard needs the columns of only two groups; other
 * counts: triangular strips).  pair_owner[fa * n_fields + fb] = the shard owning the unordered pair
 * {fa, fb} (symmetric; both latent slots of a pair, (i, field_j) and (j, field_i), live there --
 * the locality ffm.cpp:63-65,104-120 needs); lin_owner[f] = the shard that adds and updates the
 * linear terms of field f's entries (with field_map == 0 all of them sit on bias_owner, because a
 * shard then cannot tell a feature's field from its id); *bias_owner = the shard holding the bias.
 * Any output may be NULL. */
int ffm_engine_shard_plan(int32_t n_fields, int32_t n_shards, int32_t field_map, int32_t *pair_owner,
                          int32_t *lin_owner, int32_t *bias_owner);

/* The block scheduler's default block-size ramp for a learning rate (the mini-batch scheduler that
 * replaces the per-sample loop of src/task/ftrl_offline.cpp:74-83 sizes block t as
 * min(batch_size, max(1, rows_seen / ramp)): the weights a row sees are then never staler than
 * 1/ramp of the rows already learned from).  32 at the reference's default w_alpha = 1e-4 and up to
 * 1e-3; above, eight times more per decade of learning rate -- 256 at 0.01, 2048 at w_alpha = 0.1
 * --, which keeps train and eval logloss within 1e-4 of the sequential loop at the rates where
 * weights really move (tests/test_gpu_scale.py pins both ends; at alpha = 0.1 a ramp of 32 is off
 * by 5e-4 and one of 689 still by 1.5e-4 on the held-out rows). */
int32_t ffm_engine_default_batch_ramp(float w_alpha);

/* Row length of the (logical) latent arrays: n_fields*n_factors (FFM), n_factors (FM), 0 (LR). */
int64_t ffm_engine_row_len(const ffm_engine *e);

/* Replaces direct access to the public members bias / lin_w / vec_w (ftrl_model.h:35-37,
 * ffm.h:25, fm.h:20).  Host arrays, row-major [feat][row_len] = the reference's save order
 * (ffm.cpp:138-146).  Any pointer may be NULL to skip that part.  Synchronous. */
int ffm_engine_set_weights(ffm_engine *e, const float *bias, const float *lin_w, const float *vec_w);
int ffm_engine_get_weights(ffm_engine *e, float *bias, float *lin_w, float *vec_w);

/* The FTRL accumulators (protected/private in the reference: ftrl_model.h:45-48, ffm.h:30-31,
 * fm.h:25-26); needed for injected-state parity tests and resumable checkpoints. */
int ffm_engine_set_state(ffm_engine *e, const float *bias_n, const float *bias_z,
                         const float *lin_n, const float *lin_z, const float *vec_n,
                         const float *vec_z);
int ffm_engine_get_state(ffm_engine *e, float *bias_n, float *bias_z, float *lin_n, float *lin_z,
                         float *vec_n, float *vec_z);

/* The same access for a LIST of features instead of the whole model: row j of every array is
 * feature feat_ids[j] (lin_* [n], vec_* [n][row_len], host arrays, any may be NULL).  What a test
 * at the headline size (33 M features: the dense arrays above would be 82 GB each) injects and
 * reads back, and the natural primitive for checkpoint deltas.  Ids must be in [0, n_feats).
 * Synchronous. */
int ffm_engine_get_rows(ffm_engine *e, int32_t n, const int32_t *feat_ids, float *lin_w,
                        float *lin_n, float *lin_z, float *vec_w, float *vec_n, float *vec_z);
int ffm_engine_set_rows(ffm_engine *e, int32_t n, const int32_t *feat_ids, const float *lin_w,
                        const float *lin_n, const float *lin_z, const float *vec_w,
                        const float *vec_n, const float *vec_z);

/* Which features no longer hold what ffm_engine_create gave them: feature i is CHANGED when any 32-bit
 * pattern of lin_w[i], lin_n[i], lin_z[i] or of its latent record (n, z, w) differs from the create-time
 * one -- zero bits for n and z, ffm_engine_init_weights_host's draw for w (zero bits under
 * FFM_FLAG_SKIP_INIT).  Patterns, not values (-0.0f and NaN count as changed); exact whatever touched
 * the model (training, set_rows, set_weights, fill_state, the learning variant).  One device pass over
 * the model (csrc/kernels_scan.h) fills a bitmap, the host expands it: ids[0 .. *n_changed) ascending.
 * *n_changed is always set; ids == NULL only counts; cap < *n_changed with ids != NULL is
 * FFM_E_CAPACITY.  Blocks handed over by the pipelined entry points and not trained yet are trained
 * first (as ffm_engine_train_flush would; their losses stay in the flush's sum), and what the device
 * flagged since the last report is returned (and cleared) as by ffm_engine_sync -- a refused block is an
 * error here, not a model that silently lacks it.  Whole-model engines only: FFM_E_UNSUPPORTED when
 * n_shards > 1.  Synchronous.
 *   What it serves: the reference's persistence writes w only and densely (src/model/ffm.cpp:138-200,
 * lr.cpp:26-39), and SURVEY.md 8(f) rank 2 asks for checkpoints that are "actually resumable" -- a
 * fresh engine is a pure function of (seed, init_mean, init_stddev, flags), so these records
 * (ffm_engine_get_rows) plus the bias, loaded into a fresh engine of the same config with
 * ffm_engine_set_rows, reproduce the model bit for bit, and only the trained part moves. */
int ffm_engine_changed_features(ffm_engine *e, int32_t *ids, int64_t cap, int64_t *n_changed);

/* Replaces the loop over FtrlModel::train (ffm.cpp:38-49, fm.cpp:21-32, lr.cpp:9-18) in
 * FtrlOffline::one_epoch / FtrlOnline::run_task for one block of rows held in HOST memory.
 * logit_out[n_rows] receives each row's pre-update logit (train()'s return value); *loss_sum_out
 * the sum of loss(y, logit) (src/include/eval/loss.h:8-12, double).  Either may be NULL.
 * Synchronous: buffers may be reused on return. */
int ffm_engine_train_batch(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr,
                           const int32_t *field, const int32_t *feat, const float *val,
                           const int32_t *label, float *logit_out, double *loss_sum_out);

/* Replaces the loop over FtrlModel::predict (ffm.cpp:51-55, fm.cpp:34-38, lr.cpp:20-24) in
 * Evaluator::run_task / the eval branch of one_epoch.  Uses the STORED w (no lazy refresh).
 * out[n_rows] = logit, or sigmoid(logit) when output_prob != 0; label may be NULL, otherwise
 * *loss_sum_out = sum of loss(y, logit). */
int ffm_engine_predict_batch(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr,
                             const int32_t *field, const int32_t *feat, const float *val,
                             const int32_t *label, int32_t output_prob, float *out,
                             double *loss_sum_out);

/* Same two calls for blocks already resident in HBM (all pointers are DEVICE pointers, including
 * logit_out[n_rows] float and loss_sum_out[1] double; either output may be NULL).  Asynchronous on
 * the engine's stream; nnz is row_ptr[n_rows], passed so the host never reads device memory.
 * A row with more than max_row_nnz entries cannot be seen by the host here: the device detects it
 * before the block touches the model, the WHOLE block is then skipped (its outputs are NaN), and
 * the next ffm_engine_sync / ffm_engine_check_errors / ffm_engine_train_flush returns
 * FFM_E_CAPACITY.  (The host-buffer entry points check row lengths up front.) */
int ffm_engine_train_batch_device(ffm_engine *e, int32_t n_rows, int32_t nnz,
                                  const int32_t *row_ptr, const int32_t *field,
                                  const int32_t *feat, const float *val, const int32_t *label,
                                  float *logit_out, double *loss_sum_out);
int ffm_engine_predict_batch_device(ffm_engine *e, int32_t n_rows, int32_t nnz,
                                    const int32_t *row_ptr, const int32_t *field,
                                    const int32_t *feat, const float *val, const int32_t *label,
                                    int32_t output_prob, float *out, double *loss_sum_out);

/* Prediction on a sharded engine (n_shards > 1), split like training: phase 1 is
 * ffm_engine_predict_batch_device with label = NULL, output_prob = 0, loss_sum_out = NULL -- `out`
 * then receives this shard's PARTIAL logits (shard 0 adds bias + linear); the caller sums them
 * across shards (the same all-reduce as in training); phase 2 turns the full logits into what
 * predict() returns: out[i] = logit or sigmoid(logit) (ffm.cpp:51-55), and the sum of
 * loss(y, logit) (eval/loss.h:8-12) when label is given.  Device pointers; `out` may alias
 * `logit`.  Works on unsharded engines too. */
int ffm_engine_predict_finish_device(ffm_engine *e, int32_t n_rows, const float *logit,
                                     const int32_t *label, int32_t output_prob, float *out,
                                     double *loss_sum_out);

/* Pipelined training from host buffers -- what a trainer that only needs the epoch's loss calls
 * (FtrlOffline::one_epoch, src/task/ftrl_offline.cpp:74-83, accumulates loss(y, logit) and nothing
 * else).  Each call copies the block into a pinned staging slot (the caller's arrays are reusable
 * on return), uploads and groups it on a side stream, and starts training the block handed over
 * by the PREVIOUS call -- so the upload and grouping of block t and the caller's preparation of
 * block t+1 overlap the training of block t-1.  Blocks train in the order they were passed;
 * results are those of ffm_engine_train_batch called block by block.  ffm_engine_train_flush
 * trains the last block, waits, and returns (and resets) the sum of the losses of all blocks since
 * the previous flush.  Do not mix with other training / predict calls before the flush. */
int ffm_engine_train_batch_async(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr,
                                 const int32_t *field, const int32_t *feat, const float *val,
                                 const int32_t *label);
int ffm_engine_train_flush(ffm_engine *e, double *loss_sum_out);
/* The same for a trainer that gathers its blocks in PAGE-LOCKED memory (hipHostMalloc, or
 * ffm_engine_pin_host on its own buffers; every array 16-byte aligned): nothing is copied on the
 * host, the device pulls the rows straight out of the caller's arrays, and the pipeline is three
 * blocks deep -- block t+2 uploads and is grouped while block t trains.  The price: the arrays of a
 * block must stay untouched until it has been uploaded, i.e. until ffm_engine_blocks_pulled() has
 * reached the block's ordinal (blocks handed over so far, through this call or the copying one,
 * counted from 1) -- a ring of five or six blocks never waits.  Same results, same flush. */
int ffm_engine_train_batch_async_pinned(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr,
                                        const int32_t *field, const int32_t *feat, const float *val,
                                        const int32_t *label);

/* Pipelined evaluation from host buffers -- Evaluator::run_task (src/eval/evaluate.cpp:23-33) and the
 * eval branch of FtrlOffline::one_epoch (ftrl_offline.cpp:79-80) accumulate loss(y, predict(x)) and
 * nothing else: the block is uploaded through a staging slot on the side stream (zero_copy as in
 * ffm_engine_stage_batch: page-locked arrays pulled in place, untouched until
 * ffm_engine_blocks_pulled() has reached the block's ordinal) and predicted on the engine's stream,
 * so the upload of block t+1 and the caller's parsing of block t+2 overlap the forward pass of
 * block t.  Returns at once; ffm_engine_train_flush waits and returns (and resets) the sum of the
 * losses of all blocks since the previous flush.  Unsharded engines; not to be mixed with staged
 * training blocks that have not trained yet. */
int ffm_engine_predict_batch_async(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr,
                                   const int32_t *field, const int32_t *feat, const float *val,
                                   const int32_t *label, int32_t zero_copy);
/* The same, and the block's predictions come back, one float per row, without a wait:
 *   scores_host[n_rows]: page-locked, device-mapped host memory (hipHostMalloc, hipHostRegister or
 * ffm_engine_pin_host), 16-byte aligned.  It receives what ffm_engine_predict_batch(..., output_prob,
 * out, ...) puts in `out` for the same rows and model state, bit for bit (logits, or probabilities when
 * output_prob != 0).  A kernel on the engine's stream writes them right behind the block's predict
 * kernel -- exactly n_rows floats and nothing behind them -- and then publishes the block's number.
 *   scores_host == NULL is exactly ffm_engine_predict_batch_async: no extra launch, no allocation,
 * output_prob is ignored.  Loss accumulation, the flush sum, the eval metrics channel and the
 * deferral by one call are the same with and without scores.
 *   Numbering: a block's number is its 1-based staging number, the one ffm_engine_blocks_pulled()
 * counts in -- one numbering, two questions (is the block uploaded? are its scores back?).
 * ffm_engine_blocks_scored() is non-blocking and never decreases; once it has reached a block's
 * number, that block's n_rows floats are complete and visible to the host.  Blocks passed without a
 * score buffer publish nothing (the count moves from scored block to scored block).  Since a
 * block's predict launch is deferred by one call, blocks_scored() reaches block t only after the
 * call for block t+1 (or any engine call that launches the deferred block: ffm_engine_sync,
 * ffm_engine_train_flush, ...).  After ffm_engine_sync or ffm_engine_train_flush has returned, every
 * score requested so far is written and blocks_scored() has reached the last scored block.  A block
 * with n_rows == 0 is accepted and still publishes its number, in order.
 *   Refused with FFM_E_INVALID and a message: a scores_host that is not 16-byte aligned or not
 * page-locked, a sharded engine, staged training blocks still waiting (as for the call above).
 *   An error of the deferred launch of block t is returned by the engine call that made the launch
 * -- the next one --, its text prefixed with "deferred predict_batch_async block t". */
int ffm_engine_predict_batch_async_scores(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr,
                                          const int32_t *field, const int32_t *feat, const float *val,
                                          const int32_t *label, int32_t zero_copy, int32_t output_prob,
                                          float *scores_host);
int64_t ffm_engine_blocks_scored(ffm_engine *e);

/* The two halves of ffm_engine_train_batch_async, for callers that put something between forward
 * and update -- the sharded trainer's all-reduce: ffm_engine_stage_batch copies the host block into
 * a pinned staging slot, uploads it and groups it on the side stream (returns at once; the
 * caller's arrays are reusable; FFM_E_CAPACITY when three staged blocks are already waiting);
 * ffm_engine_train_forward_staged runs phase 1 of ffm_engine_train_forward_device on the OLDEST
 * staged block (partial_logit: device, may be NULL), to be followed by
 * ffm_engine_train_update_device; ffm_engine_train_staged is the whole step
 * (ffm_engine_train_batch_device: logit_out / loss_sum_out are DEVICE pointers, may be NULL) on the
 * oldest staged block of an unsharded engine.  So rows stream host -> HBM inside the training loop
 * on every rank, overlapped with the previous block's training.
 *   zero_copy != 0: the five arrays are page-locked host memory (hipHostMalloc, hipHostRegister or
 * ffm_engine_pin_host), each 16-byte aligned, and the caller leaves them untouched until the
 * block has been uploaded -- ffm_engine_blocks_pulled() (non-blocking) has reached the block's
 * 1-based staging number, or ffm_engine_sync has returned:
 * the device pulls them straight from there (a kernel reading the mapped host memory), without the
 * copy into the engine's own staging slot -- the host's share of one 8192 x 39 block drops from a
 * 3.9 MB memcpy to one kernel launch. */
int ffm_engine_stage_batch(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr,
                           const int32_t *field, const int32_t *feat, const float *val,
                           const int32_t *label, int32_t zero_copy);
int64_t ffm_engine_blocks_pulled(ffm_engine *e);
int ffm_engine_train_forward_staged(ffm_engine *e, float *partial_logit);
int ffm_engine_train_staged(ffm_engine *e, float *logit_out, double *loss_sum_out);
/* hipHostRegister / hipHostUnregister for callers that do not link the HIP runtime themselves.
 * Give it ranges that own their pages (page-aligned, whole pages: mmap, posix_memalign): the
 * runtime locks whole pages, and a range in the middle of a heap shares its first and last page
 * with whatever the allocator placed next to it. */
int ffm_engine_pin_host(void *p, size_t bytes);
int ffm_engine_unpin_host(void *p);

/* Optional look-ahead of the mini-batch scheduler: start grouping the NEXT block by feature (the
 * integer-only first stage of training) on a side stream while the current block is still being
 * updated.  The arrays must be complete in device memory when this is called and must be the very
 * ones passed to the following ffm_engine_train_batch_device / train_forward_device call (same
 * pointers and sizes); if a different block is trained next the look-ahead is discarded.  Up to
 * three blocks can be prepared ahead; they are consumed in the order they were prepared.  (Two
 * ahead is what hides the grouping: the grouping of block t+2 is scheduled to start when block
 * t-1 ends, runs beside block t's refresh and row phases and has until block t+1 ends.  Prepare
 * block t+2 BEFORE enqueuing block t's training to get that schedule.)  FFM_E_CAPACITY when
 * three prepared blocks are already waiting. */
int ffm_engine_prepare_device(ffm_engine *e, int32_t n_rows, int32_t nnz, const int32_t *row_ptr,
                              const int32_t *field, const int32_t *feat, const float *val);

/* Split-phase training for field-pair sharding over several GPUs (n_shards > 1): phase 1 groups
 * the block, refreshes this shard's weights and writes this shard's PARTIAL logits (shard 0 adds
 * bias + linear) to partial_logit[n_rows] (device); the caller sums them across shards (one RCCL
 * all-reduce of n_rows floats); phase 2 takes the summed logits and applies the updates this shard
 * owns.  ffm_engine_train_batch_device == phase 1 + phase 2 with n_shards == 1. */
int ffm_engine_train_forward_device(ffm_engine *e, int32_t n_rows, int32_t nnz,
                                    const int32_t *row_ptr, const int32_t *field,
                                    const int32_t *feat, const float *val, const int32_t *label,
                                    float *partial_logit);
int ffm_engine_train_update_device(ffm_engine *e, const float *logit, float *logit_out,
                                   double *loss_sum_out);

/* ---- several GPUs in ONE process: a group of field-pair shards --------------------------------
 * The reference has no counterpart ("distributed communication backend: none"); this
 * is what its caller FtrlOffline::one_epoch (src/task/ftrl_offline.cpp:63-103) drives when the
 * model is sharded over the GPUs of a node (BASELINE.json config 5).  ffm_group_create makes one
 * engine per entry of device_ids[n] (cfg->n_shards = n is implied, shard_rank = position; with
 * cfg->field_start every shard stores only its own slots) and one RCCL communicator per device
 * (librccl.so, bound at run time; ncclCommInitAll).  A training block is staged on EVERY engine
 * (each GPU pulls it from the caller's page-locked arrays, or from its own pinned copy), every
 * engine computes the partial logits of its field pairs, ONE ncclAllReduce(sum, float32, n_rows)
 * per block runs on the engines' own streams (ncclGroupStart/End around the n calls), every engine
 * updates its slots.  Same pipelining, ordinals and flush semantics as the one-engine entry points
 * of the same names.  Results: the one-engine results up to the association order of the
 * cross-shard logit sum (rtol 1e-5 per logit).
 *   Engines that SHARE a device (device_ids with repeats: a one-GPU dry run of the orchestration,
 * tests/test_gpu_group.py) cannot be RCCL ranks; their partial logits are summed by a kernel on
 * that device instead -- ffm_group_collective() says which of the two a group uses. */
typedef struct ffm_group ffm_group;
int ffm_group_create(const ffm_engine_config *cfg, int32_t n, const int32_t *device_ids, ffm_group **out);
void ffm_group_destroy(ffm_group *g);
int32_t ffm_group_size(const ffm_group *g);
ffm_engine *ffm_group_engine(ffm_group *g, int32_t rank);
const char *ffm_group_collective(const ffm_group *g); /* "rccl" | "device-local sum" */
/* one block, synchronous: logits (host, may be NULL) and the sum of loss(y, logit) */
int ffm_group_train_batch(ffm_group *g, int32_t n_rows, const int32_t *row_ptr, const int32_t *field,
                          const int32_t *feat, const float *val, const int32_t *label,
                          float *logit_out, double *loss_sum_out);
/* pipelined (ffm_engine_train_batch_async / _pinned): zero_copy != 0 for page-locked arrays */
int ffm_group_train_batch_async(ffm_group *g, int32_t n_rows, const int32_t *row_ptr,
                                const int32_t *field, const int32_t *feat, const float *val,
                                const int32_t *label, int32_t zero_copy);
int ffm_group_train_flush(ffm_group *g, double *loss_sum_out);
int64_t ffm_group_blocks_pulled(ffm_group *g); /* blocks every engine has uploaded */
/* predict(), synchronous: out (host, may be NULL) and the loss sum when label is given */
int ffm_group_predict_batch(ffm_group *g, int32_t n_rows, const int32_t *row_ptr, const int32_t *field,
                            const int32_t *feat, const float *val, const int32_t *label,
                            int32_t output_prob, float *out, double *loss_sum_out);

/* ---- Sample weights: one float32 per training row ------------------------------------------------
 * The reference has none (ffm.cpp:38-49 takes a Sample{x, y}); click logs are trained with the
 * negatives down-sampled (python/generate_data.py has the option), and the correction is an importance
 * weight per row or per class.  Every training entry point has a twin that takes
 * `const float *weight` -- weight[n_rows], placed after `label` -- and is otherwise its twin.
 *   gradient   tmp_grad[r] = (sigmoid(logit[r]) - (float)y[r]) * weight[r]: ONE fp32 multiply, after the
 *              subtraction, never contracted.  Nothing else of the update changes: every (n, z) step of
 *              the row takes this scalar where it took the unweighted one.  FFM_FLAG_LEARN composes:
 *              its gradient is scaled the same way.
 *   forward    weights do not touch it: the lazy refresh, the logit and logit_out are what they are
 *              without weights.  A row of weight 0 still refreshes what it touches and still returns
 *              its logit; it only contributes zero gradients.
 *   loss       the row's term is (double)weight[r] * loss(y, logit), summed in the same fixed order;
 *              the entry points (and ffm_engine_train_flush / ffm_group_train_flush) return this
 *              weighted sum.  Normalising it -- by sum(weight), say -- is the caller's.
 *   NULL       weight == NULL is exactly the unweighted call: no extra launch, no allocation, no byte
 *              moved.  An array of all 1.0f gives bit-identical state, logits and loss sum to NULL
 *              (both products are exact).  Weighted and unweighted blocks may be mixed in one pipeline.
 *   checks     the entry points that take HOST arrays (zero_copy included) check the weights on the
 *              caller's thread before anything of the block is queued: a NaN, infinite or negative
 *              weight is FFM_E_INVALID with a message, and the model is untouched.  A zero_copy weight
 *              array must be page-locked and 16-byte aligned like the other five, and stays untouched
 *              until ffm_engine_blocks_pulled() has reached the block.  The _device entry points do
 *              not inspect weights (they do not inspect val either).
 *   metrics    FFM_METRIC_TRAIN keeps counting rows, not weights.  Prediction and evaluation take no
 *              weights.  Weights are not model state: nothing of them is kept after the block's update.
 * ffm_engine_train_forward_device_weighted: the weights (device) are remembered with the pending
 * block and used by ffm_engine_train_update_device, whether the logits are its own or summed outside;
 * they must stay valid until that update has run.  ffm_engine_stage_batch_weighted: the weights travel
 * with the block (a sixth array of the upload, kept in the staging slot until the block's update has
 * run, as its labels are); ffm_engine_train_staged / train_forward_staged pick them up.
 * ffm_engine_train_batch_async_weighted covers both pipelines: zero_copy == 0 is
 * ffm_engine_train_batch_async, zero_copy != 0 ffm_engine_train_batch_async_pinned. */
int ffm_engine_train_batch_weighted(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr,
                                    const int32_t *field, const int32_t *feat, const float *val,
                                    const int32_t *label, const float *weight, float *logit_out,
                                    double *loss_sum_out);
int ffm_engine_train_batch_device_weighted(ffm_engine *e, int32_t n_rows, int32_t nnz,
                                           const int32_t *row_ptr, const int32_t *field,
                                           const int32_t *feat, const float *val, const int32_t *label,
                                           const float *weight, float *logit_out, double *loss_sum_out);
int ffm_engine_train_forward_device_weighted(ffm_engine *e, int32_t n_rows, int32_t nnz,
                                             const int32_t *row_ptr, const int32_t *field,
                                             const int32_t *feat, const float *val, const int32_t *label,
                                             const float *weight, float *partial_logit);
int ffm_engine_stage_batch_weighted(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr,
                                    const int32_t *field, const int32_t *feat, const float *val,
                                    const int32_t *label, const float *weight, int32_t zero_copy);
int ffm_engine_train_batch_async_weighted(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr,
                                          const int32_t *field, const int32_t *feat, const float *val,
                                          const int32_t *label, const float *weight, int32_t zero_copy);
int ffm_group_train_batch_weighted(ffm_group *g, int32_t n_rows, const int32_t *row_ptr, const int32_t *field,
                                   const int32_t *feat, const float *val, const int32_t *label,
                                   const float *weight, float *logit_out, double *loss_sum_out);
int ffm_group_train_batch_async_weighted(ffm_group *g, int32_t n_rows, const int32_t *row_ptr,
                                         const int32_t *field, const int32_t *feat, const float *val,
                                         const int32_t *label, const float *weight, int32_t zero_copy);

/* Measurement utility: overwrite ALL accumulators with a reproducible "warm" state drawn on the
 * device -- n ~ U[n_lo, n_hi), z ~ N(0, z_stddev) for bias, linear and latent -- so that
 * benchmarks exercise the full arithmetic (a fresh model has n = z = 0 everywhere, which makes
 * every weight take the |z| <= l1 early exit).  Not used by training itself. */
int ffm_engine_fill_state(ffm_engine *e, uint64_t seed, float n_lo, float n_hi, float z_stddev);

/* Self-test utility: y[i] = the device's sigmoid(x[i]) (utils::sigmoid<float>, utils.h:20-23, with
 * the C library's expf restated on the device); host arrays.  Lets tests compare it with the
 * host libm on millions of inputs. */
int ffm_engine_eval_sigmoid(ffm_engine *e, int32_t n, const float *x, float *y);

/* Blocks until everything queued on the engine's stream has finished; returns (and clears) the
 * error the device raised since the last report, if any -- see the _device entry points. */
int ffm_engine_sync(ffm_engine *e);
int ffm_engine_check_errors(ffm_engine *e); /* the same, named for what device callers use it for */

/* The hipStream_t the engine's kernels run on (cfg->stream, or the one it created): callers that
 * run their own work between two engine calls -- the all-reduce between train_forward_device and
 * train_update_device -- order it against this stream. */
void *ffm_engine_stream(ffm_engine *e);

/* Timing of the dominant kernel, measured with HIP events on the engine's stream around every
 * launch since the last reset (used by bench.py's roofline line). */
int ffm_engine_profile_enable(ffm_engine *e, int32_t on);
int ffm_engine_profile_read(ffm_engine *e, int32_t *n_launches, double *total_ms,
                            char *kernel_name, size_t kernel_name_cap);
/* Every timed launch costs two event records on its stream (measured: ~9 % of the step when all
 * ~17 launches are timed).  After a warm-up with everything timed, this keeps only the kernel that
 * has dominated so far and drops the other timers (and what was recorded). */
int ffm_engine_profile_focus(ffm_engine *e);
/* Text table (one line per kernel: launches, total ms, average us) into buf. */
int ffm_engine_profile_dump(ffm_engine *e, char *buf, size_t cap);

/* ---- Metrics: AUC accumulated on the device -----------------------------------------------------
 * The reference reports mean logloss and nothing else (ftrl_offline.cpp:101-102, evaluate.cpp:39-49).
 * Ranking quality is what click-through-rate models are compared by, and the pipelined entry points
 * return nothing per row on purpose -- so the engine can keep a histogram of its own scores in HBM:
 * two independent channels, both off by default (off: no launch, no allocation, nothing else changes).
 *   FFM_METRIC_EVAL  takes every labelled predict: ffm_engine_predict_batch[_device / _async] and
 *                    ffm_engine_predict_finish_device with label != NULL (so ffm_group_predict_batch).
 *   FFM_METRIC_TRAIN takes the PRE-update logits of every training block (progressive validation),
 *                    in ffm_engine_train_update_device -- the engine's own logit or, on a shard, the
 *                    summed `logit` argument -- which every training entry point ends in.
 * Definition (part of the contract):
 *   score   p = sigmoid(logit) in fp32: the bits predict(..., output_prob = 1) returns.
 *   bin     bin(p) = min((int)(p * 1048576.0f), 1048575): the product is an fp32 multiply by a power of
 *           two, hence exact; the conversion truncates; FFM_METRIC_BINS = 2^20 bins; p = 1.0f (logit
 *           +inf, or saturated) goes to the last bin, p = 0 to bin 0.
 *   NaN     a NaN score goes into no bin and is counted in n_nan (the NaNs of ffm.cpp:118, and the
 *           NaN outputs of a block the device voided).
 *   class   a row is positive iff label > 0.
 *   state   per channel pos[BINS] and neg[BINS], unsigned 64-bit counters in HBM (16 MiB), and one
 *           n_nan counter; allocated when the channel is first turned on, freed by ffm_engine_destroy.
 *           Integer counts: the result does not depend on the order rows arrive in.
 *   numbers on the host, exact integer arithmetic in a 128-bit accumulator (csrc/metrics_host.h):
 *           P = sum pos_b, N = sum neg_b, T = sum_b pos_b * neg_b (the mixed-bin tie mass),
 *           U2 = 2 * sum_b pos_b * (sum_{c<b} neg_c) + T,
 *           auc = (double)U2 / (double)(2 P N), auc_slack = (double)T / (double)(2 P N);
 *           with P * N == 0 both are NaN and the call still succeeds.  n_mixed_bins = bins that hold
 *           rows of both classes.
 *   guarantee  the exact rank AUC of the p values (ties counted 1/2) lies in
 *           [auc - auc_slack, auc + auc_slack], and equals auc when no bin holds two distinct scores
 *           of opposite labels. */
enum { FFM_METRIC_EVAL = 0, FFM_METRIC_TRAIN = 1 };
#define FFM_METRIC_BINS (1 << 20)
typedef struct { int64_t n_pos, n_neg, n_nan, n_mixed_bins; double auc, auc_slack; } ffm_metrics;
/* bit c of channel_mask = channel c on.  A channel that turns on starts from zero; one that stays on
 * keeps its counts; one that turns off stops counting (reading it is then FFM_E_INVALID).  The
 * environment variable FFM_ENGINE_METRICS=<mask>, read by ffm_engine_create, turns channels on at
 * create (of a group: on rank 0's engine). */
int ffm_engine_metrics_enable(ffm_engine *e, int32_t channel_mask);
/* The channel's numbers so far; reset != 0 also zeroes its counters.  Like every entry point it first
 * launches an evaluation block ffm_engine_predict_batch_async deferred, then waits for the engine's
 * stream.  It does NOT train blocks that are staged and not trained yet: a caller that wants every
 * block it handed over counted calls ffm_engine_train_flush first.  A channel that is off:
 * FFM_E_INVALID. */
int ffm_engine_metrics_read(ffm_engine *e, int32_t channel, int32_t reset, ffm_metrics *out);
/* The raw counters: pos / neg are host arrays of FFM_METRIC_BINS (either may be NULL).  Same waits. */
int ffm_engine_metrics_histogram(ffm_engine *e, int32_t channel, uint64_t *pos, uint64_t *neg);
/* The reduction alone: pure host arithmetic, no engine, no device; any n_bins >= 0. */
int ffm_engine_metrics_from_histogram(const uint64_t *pos, const uint64_t *neg, int64_t n_bins,
                                      int64_t n_nan, ffm_metrics *out);
/* A group's labels are seen by every rank; rank 0's engine keeps the channels. */
int ffm_group_metrics_enable(ffm_group *g, int32_t channel_mask);
int ffm_group_metrics_read(ffm_group *g, int32_t channel, int32_t reset, ffm_metrics *out);

/* Keyed capture: the grouped AUC (GAUC).  A global AUC mixes how well the model orders the rows ONE user,
 * request or placement sees -- what serving does -- with how well it tells keys of a high click rate
 * from keys of a low one, which no ranker can use.  GAUC takes the AUC inside each key and averages
 * those, weighted by impressions.  Keyed capture is independent of the histogram channels above and
 * uses the same channel numbers; it is off until ffm_engine_metrics_key_field turns it on (off: no
 * launch, no allocation).
 *   FFM_METRIC_EVAL  takes every labelled block that passes through ffm_engine_predict_batch_device:
 *                    the copying, async, async-scores and deferred forms all end in it.
 *   FFM_METRIC_TRAIN takes the pre-update logits in ffm_engine_train_update_device, where the
 *                    histogram channel takes them.
 *   ffm_engine_predict_finish_device has no rows, hence no keys: it is NOT captured.
 * Definition (part of the contract), per captured row:
 *   key     the feat of the first entry in row order with field == key_field and 0 <= feat < n_feats,
 *           as the kernels see it: after FFM_FLAG_HASH_IDS, so ids that collide there merge their keys.
 *           A row with no such entry counts in n_unkeyed and is left out.
 *   score   p = sigmoid(logit) in fp32, the bits output_prob = 1 returns.  A NaN p counts in n_nan and
 *           is left out.
 *   class   the row is positive iff label > 0.
 *   state   one 64-bit word per captured row, key << 32 | (bits of p) << 1 | class, in a buffer of
 *           capacity_rows words in HBM, allocated (with a scratch buffer of the same size and the per-key
 *           table) when capture is turned on, freed by ffm_engine_destroy.  A row that arrives when the
 *           buffer is full is not stored and counts in n_overflow.
 *   per key g, in exact integers: P_g, N_g = its positive / negative rows;
 *           U2_g = sum over its positives of (2 * #{neg of g with smaller p} + #{neg of g with equal p}).
 *   over the captured rows, on the host in double, keys ascending, one running sum each, in this order:
 *           auc_g = (double)U2_g / (2.0 * (double)P_g * (double)N_g)     for keys with P_g * N_g > 0 only
 *           num += (double)(P_g + N_g) * auc_g;   den += (double)(P_g + N_g);
 *           gauc = num / den, NaN when den == 0 (the call still succeeds).
 *   The result does not depend on the order rows arrive in (which rows a full buffer turns away does).
 *   n_rows = rows stored, n_keys = distinct keys among them, n_keys_mixed / n_rows_mixed = the keys with
 *   rows of both classes and their rows (den).
 * Out of scope: groups and shards (every ffm_group_* engine, n_shards > 1), LR and FM (no fields) --
 * all FFM_E_UNSUPPORTED; a per-row key array passed by the caller; weighting other than by impressions
 * (ffm_engine_metrics_keyed_table hands out the integers for any other); an exact global AUC.  Serving
 * engines are allowed: they predict. */
typedef struct { int64_t n_rows, n_keys, n_keys_mixed, n_rows_mixed, n_nan, n_unkeyed, n_overflow; double gauc; } ffm_keyed_metrics;
/* bit c of channel_mask = capture on channel c on, with this key field and capacity.  A channel that
 * turns on starts empty; one that stays on keeps its rows unless key_field or capacity_rows changed,
 * which empties it.  channel_mask == 0 turns capture off and frees nothing (the other two arguments
 * are then ignored).  key_field outside [0, n_fields) or capacity_rows <= 0: FFM_E_INVALID;
 * capacity_rows above 2^30: FFM_E_UNSUPPORTED. */
int ffm_engine_metrics_key_field(ffm_engine *e, int32_t channel_mask, int32_t key_field, int64_t capacity_rows);
/* The channel's numbers so far: sorts the captured words and ranks them on the device, averages on the
 * host.  Waits as ffm_engine_metrics_read does (a deferred evaluation block first, then the stream);
 * reset != 0 empties the buffer and the three counters after the snapshot, on the stream.  A channel
 * whose capture is off: FFM_E_INVALID. */
int ffm_engine_metrics_read_keyed(ffm_engine *e, int32_t channel, int32_t reset, ffm_keyed_metrics *out);
/* The per-key integers, keys ascending: key[g], pos[g] = P_g, neg[g] = N_g, u2[g] = U2_g for g < *n_keys.
 * cap = the arrays' length; too small: FFM_E_CAPACITY with *n_keys set (any array may be NULL with
 * cap == 0 to ask for the count).  Same waits, no reset. */
int ffm_engine_metrics_keyed_table(ffm_engine *e, int32_t channel, int64_t cap, int32_t *key, int64_t *pos, int64_t *neg,
                                   uint64_t *u2, int64_t *n_keys);
/* The average alone: pure host arithmetic, no engine, no device; n_nan, n_unkeyed, n_overflow come out 0. */
int ffm_engine_metrics_from_keyed(const int64_t *pos, const int64_t *neg, const uint64_t *u2, int64_t n_keys,
                                  ffm_keyed_metrics *out);

/* ---- Hashed ids: FFM_FLAG_HASH_IDS ----------------------------------------------------------------
 * The reference erases every entry whose id is not in [0, n_feats) (remove_out_range, ftrl_model.cpp:36-42,
 * ffm.cpp:30-36); real click logs come with one global id space, fields interleaved, often larger than the
 * model one can afford.  With this flag the engine applies the hashing trick, per field, to every block of
 * HOST rows: the model then sees id' where the caller wrote feat.  The mapping (csrc/hash_ids.h; unsigned
 * 32-bit wrap-around arithmetic except the last step) is part of the contract:
 *   salt = (uint32)(field + 1) * 0x9e3779b9                     (LR / FM: field taken as 0)
 *   x  = (uint32)feat ^ salt
 *   x ^= x >> 16;  x *= 0x85ebca6b;  x ^= x >> 13;  x *= 0xc2b2ae35;  x ^= x >> 16
 *   id' = lo + (int32)(((uint64)x * (uint64)width) >> 32)       (multiply-high: no divide)
 *   (lo, width) = (field_start[f], field_start[f+1] - field_start[f]) for FFM with cfg->field_start,
 *                 (0, n_feats) in every other case.
 * Entries the reference erases stay erased: feat < 0 gives id' = -1, and so does, for FFM, a field outside
 * [0, n_fields).  Every non-negative id up to INT32_MAX is hashed into range.  There is no seed: the mapping
 * is a pure function of (field, feat, field_start / n_feats).  Two raw ids of one row that collide under one
 * field make a row that holds one id twice -- the serial case of DESIGN.md section 3, nothing special.
 *   create     with the flag, a field of width 0 is FFM_E_INVALID (nothing can land in it).  The environment
 *              variable FFM_ENGINE_HASH_IDS=1, read by ffm_engine_create, turns the flag on (every rank of a
 *              group), as FFM_ENGINE_METRICS does for the metrics channels.
 *   where      every entry point that takes HOST rows: training and prediction, synchronous, pipelined,
 *              page-locked / zero_copy, weighted, with scores, and the ffm_group_* calls.  The pipelined ones
 *              hash inside the upload kernel (feat and field move in one loop; no byte crosses PCIe twice), the
 *              synchronous ones by one in-place kernel behind their copies.  The caller's buffers are never
 *              written.  With field_start the hashed ids lie in their fields' ranges: compact shards accept
 *              any data, and rows of one entry per field are regular blocks.
 *   _device    the entry points that take DEVICE rows take ids as they are, as they take val as it is:
 *              their callers hash with ffm_engine_hash_ids_device -- the same kernel, asynchronous on the
 *              engine's stream; feat_out may be feat_in; field == NULL means, for FFM, rows of one entry per
 *              field in field order (entry p is field p mod n_fields); FFM_E_INVALID on an engine without
 *              the flag.
 *   host       ffm_engine_hash_ids_host is the same function of (model_type, n_feats, n_fields, field_start)
 *              on the host, bit for bit, and needs no device (field_start may be NULL; n_fields is ignored
 *              for LR / FM).
 *   ids        ffm_engine_get_rows / set_rows, get / set_weights and _state, changed_features, the model
 *              files and checkpoints all speak MODEL ids, i.e. hashed ones.
 * Without the flag nothing changes: the same kernels, the same launches, no allocation. */
int ffm_engine_hash_ids_device(ffm_engine *e, int32_t nnz, const int32_t *field, const int32_t *feat_in,
                               int32_t *feat_out);
int ffm_engine_hash_ids_host(int32_t model_type, int32_t n_feats, int32_t n_fields, const int32_t *field_start,
                             int32_t nnz, const int32_t *field, const int32_t *feat_in, int32_t *feat_out);

/* ---- Field sketches: the fields' cardinalities counted on the device, and id ranges sized by them ----
 * Under FFM_FLAG_HASH_IDS with cfg->field_start every field hashes into its own id range; how wide each range
 * should be depends on how many distinct ids the field holds, which nothing knows before the data is read.  A
 * SKETCH counts that: one HyperLogLog sketch per field, filled by one kernel from rows in host memory (or in
 * HBM) before a model exists.  It touches no engine and needs none.
 *   sketch     n_fields x M registers, M = FFM_SKETCH_REGS = 2^14, all zero at create.
 *   counting   an entry (field, feat) COUNTS iff feat >= 0 and 0 <= field < n_fields -- exactly the entries the
 *              mapping of "Hashed ids" keeps for an FFM model.  Every other entry adds one to n_bad and nothing
 *              else.  n_valid counts the counting entries.  For a counting entry
 *                x    = the 32 hashed bits of "Hashed ids" (after the last x ^= x >> 16, before the multiply)
 *                idx  = x >> 18
 *                w    = x << 14                                 (32 bits)
 *                rank = (w == 0) ? 19 : clz32(w) + 1
 *                reg[field][idx] = max(reg[field][idx], rank)
 *   fields     field == NULL: entry p of the call belongs to field p mod n_fields (rows of one entry per field
 *              in field order, as for ffm_engine_hash_ids_device).
 *   exactness  the mix is a bijection on 32 bits: distinct ids of a field are distinct x, so the estimator needs
 *              no large-range correction.  Registers are maxima and the counters integer sums: the result does
 *              not depend on the order or the batching of the entries, and two sketches fed the halves of a
 *              file hold, register by register, the maximum of what one sketch fed the whole file holds.
 *   add        zero_copy != 0: the arrays are page-locked (ffm_engine_pin_host) and the kernel reads them in
 *              place (16-byte aligned arrays move as 16-byte vectors).  Otherwise they are copied into one of two
 *              page-locked staging buffers owned by the sketch, grown on demand.  Either way the call returns
 *              once the caller may reuse the arrays; no host-to-device copy is queued, a kernel pulls the
 *              entries.  _add_device: the arrays are in device memory; asynchronous on the
 *              sketch's stream.  nnz == 0 is a no-op.  FFM_E_INVALID: feat == NULL with nnz > 0, nnz < 0,
 *              n_fields <= 0; FFM_E_DEVICE without a device.
 *   read       waits for the sketch's stream; reg may be NULL; the sketch keeps counting afterwards.
 *   estimate   pure host arithmetic, no device; in double, the registers of a field in ascending index:
 *                S = sum of 2^(-reg)          (exact: 16384 terms of at most 19 fractional bits)
 *                E = alpha * M^2 / S          alpha = 0.7213 / (1 + 1.079 / M)
 *                if E <= 2.5 * M and V > 0 registers are zero: E = M * ln(M / V)
 *              an empty field gives 0.0.  Standard error 1.04 / sqrt(M) = 0.81 %.
 *   ranges     ffm_engine_field_ranges: pure host arithmetic in exact integers.  count[f] is clamped to
 *              [1, 2^31]; a negative count, or n_feats < 2 * n_fields, is FFM_E_INVALID.
 *                base     = min(4096, n_feats / (2 * n_fields))
 *                R        = n_feats - n_fields * base,  C = sum of count
 *                width[f] = base + (R * count[f]) / C        (unsigned 64-bit; the product is below 2^63)
 *              the L ids still left over go one each to the L fields with the largest (R * count[f]) mod C,
 *              ties to the lower field.  field_start is the prefix sum: field_start[0] = 0,
 *              field_start[n_fields] = n_feats.  The floor `base` keeps a two-valued field from sharing three
 *              slots and costs at most 4096 * n_fields ids.
 * OUT OF SCOPE  groups, shards and several GPUs with ranges other than uniform ones; LR / FM, which have no
 *   fields; recording ranges in checkpoints; sketching evaluation data; choosing n_feats for the caller. */
typedef struct ffm_sketch ffm_sketch;
#define FFM_SKETCH_REGS 16384
int ffm_engine_sketch_create(int32_t n_fields, int32_t device_id, ffm_sketch **out);
int ffm_engine_sketch_add(ffm_sketch *s, int32_t nnz, const int32_t *field, const int32_t *feat, int32_t zero_copy);
int ffm_engine_sketch_add_device(ffm_sketch *s, int32_t nnz, const int32_t *field, const int32_t *feat);
int ffm_engine_sketch_read(ffm_sketch *s, uint8_t *reg /* [n_fields][REGS], may be NULL */, int64_t *n_valid, int64_t *n_bad);
void ffm_engine_sketch_destroy(ffm_sketch *s);
/* pure host arithmetic, no device: */
int ffm_engine_sketch_estimate(const uint8_t *reg, int32_t n_fields, double *distinct /* [n_fields] */);
int ffm_engine_field_ranges(const int64_t *count, int32_t n_fields, int32_t n_feats, int32_t *field_start /* [n_fields + 1] */);

/* ---- Rare ids: ids seen fewer than T times share one id per field ------------------------------------
 * A feature seen once or twice keeps a latent row that is still its random draw, adds noise to every
 * prediction that touches it after its one update, and occupies a slot of the hashed id space that frequent
 * ids then collide with.  The usual remedy (libffm's Criteo recipe: T = 10) maps every id seen fewer than T
 * times to one "rare" id per field.  Here the counting runs on the device before a model exists, and the
 * fold runs wherever an engine hashes.
 *   counter    ffm_idcount: 2^bits 32-bit words in HBM, all zero at create, plus n_valid and n_bad.  bits in
 *              [8, 30], cap in [1, 65535]; n_fields == 0 means LR / FM, and the field is taken as 0.
 *   counting   an entry (field, feat) COUNTS iff feat >= 0 and, with n_fields > 0, 0 <= field < n_fields --
 *              the entries "Hashed ids" keeps.  Every other entry adds one to n_bad and nothing else.  For a
 *              counting entry
 *                slot = x >> (32 - bits)          x = the 32 hashed bits of "Hashed ids"
 *              and the counter of slot goes up by one -- until it has reached cap: read gives min(count, cap)
 *              EXACTLY, whatever the order, the batching or the split of the entries across calls (integer
 *              sums only).  Two ids that share a slot are counted together: a rare id may be kept because
 *              of its neighbour, a frequent one is never folded.  field == NULL with n_fields > 0: entry p
 *              of the call is field p mod n_fields, as for a sketch.
 *   add        _add (zero_copy 0 / 1), _add_device, _read and _destroy: the arguments, the chunking and the
 *              refusals of the sketch's calls of the same names.
 *   keep       ffm_engine_idcount_keep: the KEEP-MAP of min_count T, 1 <= T <= cap (anything else is
 *              FFM_E_INVALID: counts above the cap are not known).  2^bits / 64 words; bit j of word i is set
 *              iff min(count[64 i + j], cap) >= T.  n_kept_slots = the set bits; n_folded_entries = the sum
 *              of the counts below T = how many counted entries the map folds (counts below cap are exact).
 *   fold       ffm_engine_set_rare_fold copies a map into HBM (words == NULL: turns the fold off and frees
 *              it).  The engine must have FFM_FLAG_HASH_IDS (else FFM_E_INVALID); training and serving engines
 *              alike; a group's or a shard's engine is FFM_E_UNSUPPORTED.  The engine must be idle: a staged
 *              block that waits to be trained, or one between train_forward and train_update, is
 *              FFM_E_INVALID; the call then waits for whatever the engine still has in flight.  The fold holds
 *              for every block handed over afterwards: a counting entry whose slot's bit is 0 has its raw id
 *              replaced by FFM_RARE_ID before the hash of "Hashed ids" runs.  Nothing else changes; erased
 *              entries stay erased.  The rare id of a field is therefore the model id of (field, FFM_RARE_ID):
 *              it lies in the field's own range under every ranges setting, and in [0, n_feats) for LR / FM.
 *              A genuine raw id INT32_MAX shares it.  No id of the model is reserved.
 *   where      everywhere an engine hashes: the upload kernel of the pipelined calls, the in-place kernel
 *              behind the synchronous copies (training, prediction, ffm_engine_score_candidates) and
 *              ffm_engine_hash_ids_device.  The other _device entry points keep taking ids as they are.
 *              An engine without a map runs the kernels, launches and kernel arguments it always ran.
 *   host       ffm_engine_fold_ids_host is the fold on the host, bit for bit, and needs no device; composed
 *              with ffm_engine_hash_ids_host it gives the model ids.  ffm_engine_rare_slots_host gives the
 *              slots (field == NULL: field 0).
 *   sketch     ffm_engine_sketch_set_filter: with a filter, an entry whose bit is 0 counts as the one id
 *              FFM_RARE_ID of its field, so counted ranges are sized by the ids that stay.  words == NULL
 *              turns it off.
 * OUT OF SCOPE  groups, shards and several GPUs; admission while training (a running count that lets an id
 *   in once it has been seen T times); recording the map or its checksum in checkpoints; counting evaluation
 *   data; choosing T for the caller. */
typedef struct ffm_idcount ffm_idcount;
#define FFM_RARE_ID 2147483647
int ffm_engine_idcount_create(int32_t n_fields, int32_t bits, int32_t cap, int32_t device_id, ffm_idcount **out);
int ffm_engine_idcount_add(ffm_idcount *s, int32_t nnz, const int32_t *field, const int32_t *feat, int32_t zero_copy);
int ffm_engine_idcount_add_device(ffm_idcount *s, int32_t nnz, const int32_t *field, const int32_t *feat);
int ffm_engine_idcount_read(ffm_idcount *s, uint32_t *counts /* [2^bits], already min(., cap), may be NULL */,
                            int64_t *n_valid, int64_t *n_bad);
int ffm_engine_idcount_keep(ffm_idcount *s, int32_t min_count, uint64_t *words /* [2^bits / 64] */,
                            int64_t *n_kept_slots, int64_t *n_folded_entries);
void ffm_engine_idcount_destroy(ffm_idcount *s);
int ffm_engine_set_rare_fold(ffm_engine *e, int32_t bits, const uint64_t *words /* [2^bits / 64] or NULL */);
int ffm_engine_sketch_set_filter(ffm_sketch *s, int32_t bits, const uint64_t *words /* [2^bits / 64] or NULL */);
/* pure host arithmetic, no device: */
int ffm_engine_fold_ids_host(int32_t n_fields, int32_t bits, const uint64_t *words, int32_t nnz, const int32_t *field,
                             const int32_t *feat_in, int32_t *feat_out);
int ffm_engine_rare_slots_host(int32_t bits, int32_t nnz, const int32_t *field, const int32_t *feat, uint32_t *slot);

/* ---- Value buckets: numeric fields as quantile buckets -------------------------------------------------
 * A numeric column (a count, a price, a dwell time) is field:one_id:value in libffm text, and the value
 * multiplies straight into the linear term and every pair term: an unbounded count scales gradients by
 * orders of magnitude, and one latent row per field cannot express a non-monotone effect.  The usual remedy
 * is quantile buckets.  Here a value histogram per field is counted on the device before a model exists, the
 * host cuts it into buckets of equal mass with exact integers, and every place an engine hashes replaces
 * (id, value) by (bucket, 1.0f).  All of it is integer work on the float's bit pattern -- no floating-point
 * instruction, so denormal modes cannot matter.
 *   key(v)     u = bits(v); if (u & 0x7fffffff) == 0 then u = 0 (-0.0 and +0.0 give one key);
 *              key = (u >> 31) ? ~u : (u | 0x80000000), which preserves the order of the values.
 *              bin(v) = key >> 16, one of FFM_BUCKET_BINS = 65536: sign, exponent and 7 mantissa bits, a
 *              relative resolution below 1 %.  NaN is (u & 0x7fffffff) > 0x7f800000; a NaN has no bin.
 *   histogram  ffm_valhist (FFM only, 1 <= n_fields <= 4096): n_fields x 65536 64-bit counters in HBM, all
 *              zero at create, plus n_valid, n_bad and n_nan.  An entry (field, val) COUNTS iff
 *              0 <= field < n_fields (n_valid); every other entry adds one to n_bad and nothing else.  A
 *              counting NaN adds one to n_nan and to no bin.  field == NULL: entry p of the call is field
 *              p mod n_fields, as for a sketch.  Counts are EXACT whatever the order, the batching or the
 *              split of the entries across calls (integer sums only).  _add (zero_copy 0 / 1), _add_device,
 *              _read and _destroy: the arguments, the chunking and the refusals of the sketch's calls.
 *   edges      ffm_engine_bucket_edges (host arithmetic): one field's counts c[0 .. 65535], N = sum c,
 *              B = n_buckets in [2, 256].  For j = 1 .. B - 1: t_j = (j N + B - 1) / B in integer division,
 *              e_j = the smallest bin whose inclusive cumulative count is >= t_j.  The edges are the e_j
 *              with repeats dropped, strictly ascending, at most FFM_BUCKET_MAX_EDGES = 255.  N == 0: no
 *              edges.  bucket(bin) = the number of edges < bin, in [0, n_edges].
 *   table      n_edges [n_fields] (-1: the field is not bucketed) and edges [n_fields][FFM_BUCKET_MAX_EDGES]
 *              (field f's edges are the first n_edges[f] of its row; the rest is not read).
 *   apply      ffm_engine_set_buckets copies a table into HBM (n_edges == NULL: takes it off and frees it).
 *              The engine must have FFM_FLAG_HASH_IDS and be FFM (else FFM_E_INVALID); training and serving
 *              engines alike; a group's or a shard's engine is FFM_E_UNSUPPORTED; edges that do not ascend
 *              strictly or n_edges > 255 are FFM_E_INVALID; the engine must be idle, as for
 *              ffm_engine_set_rare_fold.  From then on an entry (f, id, v) with id >= 0, 0 <= f < n_fields
 *              and n_edges[f] >= 0 becomes id' = bucket(bin(v)), v' = 1.0f; a NaN gives id' =
 *              FFM_BUCKET_NAN_ID = 65536.  The raw id is ignored (a numeric column has one).  A bucketed
 *              entry is NEVER rare-folded -- its id is one of at most 257 chosen by the data's own
 *              quantiles -- and then goes through the hash of "Hashed ids".  Every other entry takes the
 *              path it takes without a table: fold if there is a keep-map, then hash.  A block with
 *              val == NULL is, as ever, the block with an array of 1.0f.
 *   where      everywhere an engine hashes rows that came with (or without) their values: the upload kernel
 *              of the pipelined calls, the in-place kernel behind the synchronous copies (training,
 *              prediction, ffm_engine_score_candidates, ffm_engine_predict_ablated).
 *              ffm_engine_bucket_ids_device is the whole mapping (bucket, fold, hash) for blocks already in
 *              HBM; ffm_engine_hash_ids_device and the other _device entry points keep taking arrays as they
 *              are.  An engine without a table runs the kernels, launches and kernel arguments it always ran.
 *   host       ffm_engine_bucket_ids_host is the bucket step alone, bit for bit, and needs no device
 *              (field == NULL: entry p is field p mod n_fields; val_in == NULL: every value is 1.0f);
 *              composed with the fold of the entries it left alone and ffm_engine_hash_ids_host it gives the
 *              model ids.
 * OUT OF SCOPE  groups, shards and several GPUs; LR / FM; buckets learnt while training; keeping the value
 *   next to the bucket; recording the table in checkpoints; counting evaluation data. */
typedef struct ffm_valhist ffm_valhist;
#define FFM_BUCKET_BINS 65536
#define FFM_BUCKET_MAX_EDGES 255
#define FFM_BUCKET_NAN_ID 65536
int ffm_engine_valhist_create(int32_t n_fields, int32_t device_id, ffm_valhist **out);
int ffm_engine_valhist_add(ffm_valhist *s, int32_t nnz, const int32_t *field, const float *val, int32_t zero_copy);
int ffm_engine_valhist_add_device(ffm_valhist *s, int32_t nnz, const int32_t *field, const float *val);
int ffm_engine_valhist_read(ffm_valhist *s, uint64_t *counts /* [n_fields][FFM_BUCKET_BINS], may be NULL */,
                            int64_t *n_valid, int64_t *n_bad, int64_t *n_nan);
void ffm_engine_valhist_destroy(ffm_valhist *s);
int ffm_engine_set_buckets(ffm_engine *e, const int32_t *n_edges /* [n_fields] or NULL */,
                           const uint16_t *edges /* [n_fields][FFM_BUCKET_MAX_EDGES] */);
int ffm_engine_bucket_ids_device(ffm_engine *e, int32_t nnz, const int32_t *field, const int32_t *feat_in, const float *val_in,
                                 int32_t *feat_out, float *val_out);
/* pure host arithmetic, no device: */
int ffm_engine_bucket_edges(const uint64_t *counts /* [FFM_BUCKET_BINS] */, int32_t n_buckets,
                            uint16_t *edges /* [FFM_BUCKET_MAX_EDGES] */, int32_t *n_edges);
int ffm_engine_bucket_ids_host(int32_t n_fields, const int32_t *n_edges, const uint16_t *edges, int32_t nnz, const int32_t *field,
                               const int32_t *feat_in, const float *val_in, int32_t *feat_out, float *val_out,
                               uint8_t *bucketed /* [nnz], may be NULL */);

/* ---- Rows without values: val == NULL is 1.0f -------------------------------------------------------
 * Click logs are categorical: after hashing every entry of a libffm file is field:id:1, and an array of
 * 1.0f is a third of a block's bytes over PCIe (half of what is left once the field array stays at home).
 * On every entry point that takes rows in HOST memory, val == NULL with nnz > 0 means "every value is 1.0f"
 * (bits 0x3f800000), for LR, FM and FFM:
 *   where      ffm_engine_train_batch[_weighted], ffm_engine_predict_batch; ffm_engine_stage_batch[_weighted],
 *              ffm_engine_train_batch_async[_pinned|_weighted], ffm_engine_predict_batch_async[_scores], with
 *              zero_copy 0 and 1; ffm_group_train_batch[_async][_weighted], ffm_group_predict_batch.
 *   contract   a block handed over without values gives, bit for bit, what the same block gives with an
 *              array of 1.0f: logits, losses, w, n, z, scores and the metrics channels.
 *   combines   freely with field == NULL (where that is taken: the staged calls), sample weights, FFM_FLAG_HASH_IDS, serving engines (both formats)
 *              and FFM_FLAG_LEARN; blocks with and without values mix freely in one pipeline.
 *   how        nothing of val is copied, page-locked or read.  The pipelined calls' upload kernel writes the
 *              staging slot's value array itself (16-byte stores over its own grid stride, behind the link),
 *              again for every such block; the synchronous calls run one small fill kernel in place of the
 *              copy.  Every kernel downstream reads values as always.
 *   _device    the entry points that take DEVICE rows, and ffm_engine_prepare_device, take arrays as they
 *              are: there val == NULL with nnz > 0 stays FFM_E_INVALID.
 * A block that brings its val array runs exactly the launches, kernels and kernel arguments it ran before.
 * No new symbol, no new ABI version: callers that always pass val see no change. */

/* ---- Normalised rows: FFM_FLAG_NORM_ROWS -----------------------------------------------------------------
 * libffm and xLearn multiply every pair term by 1 / sum(v^2) of its row (their default; --no-norm switches it
 * off), which is dividing every value by the row's Euclidean length.  An engine created with
 * FFM_FLAG_NORM_ROWS does that to every block that arrives in HOST memory, on the device, behind the block's
 * upload and id rewriting and ahead of every kernel that reads val (normalize_rows_kernel, csrc/kernels_norm.h).
 * The definition, fixed so that host and device agree bit for bit -- per row, in entry order, over the entries
 * the model keeps (LR / FM: 0 <= feat < n_feats; FFM also 0 <= field < n_fields; on the ids as the kernels see
 * them: after hashing, rare folding and bucketing, a bucketed entry counting as the 1 it became):
 *     s = 0.0f
 *     for each kept entry p of the row, in order:   s = fl(s + fl(v[p] * v[p]))     two roundings, never an FMA
 *     scale = (s > 0 and s finite) ? fl(1.0f / fl(sqrt(s))) : 1.0f                  IEEE sqrt and divide, denormals kept
 *     for every entry p of the row (kept or not):   v'[p] = fl(v[p] * scale)
 *   unscaled   a row whose s is zero, infinite or NaN passes through unchanged: an empty row, a row of zeros or of
 *              erased entries only, an overflowing sum, a NaN value -- NaN rows behave as on an unflagged engine.
 *   order      the sum is sequential on purpose (what a host loop gives); a tree order gives other bits.
 *   val NULL   a block without values is normalised like the array of 1.0f it stands for.
 *   where      every entry point that takes rows in HOST memory: ffm_engine_train_batch[_weighted],
 *              ffm_engine_predict_batch, ffm_engine_predict_ablated, ffm_engine_stage_batch[_weighted],
 *              ffm_engine_train_batch_async[_pinned|_weighted], ffm_engine_predict_batch_async[_scores] (zero_copy 0
 *              and 1).  The caller's buffers are never written: with zero_copy the kernel works on the staging
 *              slot's device copy.  LR, FM and FFM; training engines and both serving formats; sample weights,
 *              FFM_FLAG_LEARN, FFM_FLAG_HASH_IDS with keep-map and buckets, field == NULL, the metrics channels and
 *              keyed capture all combine.
 *   contract   a flagged engine fed raw blocks gives, bit for bit, what an unflagged engine of the same
 *              configuration gives when fed ffm_engine_normalize_rows_host of them.
 *   ablation   ffm_engine_predict_ablated drops a field AFTER normalisation: variant v is predict_batch of the
 *              normalised block without field v; the norm is not recomputed without the field.
 *   refused    FFM_E_INVALID with a message that says so, before anything is queued: ffm_group_create with the
 *              flag; ffm_engine_create with the flag and n_shards > 1 (a shard does not own whole rows);
 *              ffm_engine_score_candidates[_device] on a flagged engine (the shared context terms would need a
 *              scale per candidate).
 *   _device    the entry points that take DEVICE rows take arrays as they are, flag or no flag.  For their callers:
 * ffm_engine_normalize_rows_device: the definition applied to a block in device memory, asynchronous on the
 *   engine's stream; val_out == val_in (in place) is allowed, val_in == NULL means ones, field is NULL for LR / FM.
 *   Works on any engine, flagged or not (the engine gives n_feats, n_fields and the model type).
 * ffm_engine_normalize_rows_host: the same in plain C++, no device needed; field == NULL on FFM: the id decides.
 * ffm_engine_norm_stats: rows that went through the kernel since create or the last reset, and how many of them
 *   were left unscaled (counted on the device, one atomic per wave); waits for the launches counted.
 * The flag is not stored in weights, model files or serving deltas: whoever scores a model trained with it passes
 * it again.  An unflagged engine launches exactly what it launched before; FFM_ENGINE_ABI_VERSION and
 * ffm_engine_config are what they were. */
int ffm_engine_normalize_rows_device(ffm_engine *e, int32_t n_rows, int32_t nnz, const int32_t *row_ptr, const int32_t *field,
                                     const int32_t *feat, const float *val_in, float *val_out);
int ffm_engine_normalize_rows_host(int32_t model_type, int32_t n_feats, int32_t n_fields, int32_t n_rows, const int32_t *row_ptr,
                                   const int32_t *field, const int32_t *feat, const float *val_in /* NULL: ones */, float *val_out);
int ffm_engine_norm_stats(ffm_engine *e, int32_t reset, int64_t *rows, int64_t *unscaled);

/* ---- Refresh: every stored weight from its accumulators -----------------------------------------
 * train() refreshes w = W(n, z) lazily, for what a row touches, BEFORE it updates (n, z), and leaves the
 * stored w alone afterwards (ffm.cpp:38-49, :72-88); predict() reads the stored w and nothing else
 * (ffm.cpp:51-55).  So what prediction, evaluation and the model files see is one update behind the
 * accumulators -- with this engine's block semantics one whole block per feature: a feature that occurred
 * in exactly one block of a run is scored as if it had never been seen, though its (n, z) hold a real
 * update.  This call makes one streaming pass over everything the engine STORES -- the bias triple, the
 * linear arrays, every latent record, by position, so a compact or full-length shard is served like a
 * whole model (csrc/kernels_refresh.h) -- and sets w = W(n, z) wherever the accumulators are live.
 * Rule per element (the contract):
 *   live     (bits(n) | bits(z)) != 0: bit patterns, so -0.0f and NaN are live.
 *   dead     w is not counted and keeps its bits (create-time draws, padding slots, slots and linear
 *            entries another shard owns).
 *   linear, bias   w_new = maybe_zero_weight(n, z) (ftrl_model.h:28-33), the bits the lazy refresh stores.
 *   latent   the same; under FFM_FLAG_LEARN a slot whose n is not > 0 keeps w_old, as its refresh does.
 *   counters live = live elements; nonzero = live and !(w_new == 0.0f) (a NaN weight counts, -0.0f does
 *            not); moved = live and bits(w_new) != bits(w_old).  lin_* cover the linear weights and the
 *            bias (on the engine that owns it), lat_* the latent elements (0 for LR).
 * (n, z) are never written.  The next training block recomputes the same w from the same (n, z) for what
 * it touches, so training after a refresh is bit-identical -- logits, losses, state -- to training without
 * it; only what prediction and persistence see changes.  The set ffm_engine_changed_features reports is
 * the same before and after: a live element was already changed, a dead one is not written.  A second
 * call right after the first moves nothing and stores nothing.
 *   Synchronous.  Before its kernel it drains as ffm_engine_changed_features does: a deferred evaluation
 * block is launched (it sees the weights as they were), blocks staged by the pipelined entry points and
 * not trained yet are trained (their losses stay in the flush's sum), the staging thread is waited for,
 * and what the device flagged since the last report is returned and cleared here.  Works on sharded
 * engines; one whose group still holds staged blocks is refused (FFM_E_INVALID) -- the group's call trains
 * them first.  ffm_group_refresh_weights runs every shard; every slot that can be live belongs to exactly
 * one shard, so its counters are plain sums and equal those of the unsharded model.  out may be NULL.
 * The counter buffer (48 bytes of HBM) is allocated by the first call and freed by ffm_engine_destroy: an
 * engine that never calls this allocates nothing, launches nothing and changes in nothing. */
typedef struct { int64_t lin_live, lin_nonzero, lin_moved, lat_live, lat_nonzero, lat_moved; } ffm_refresh_stats;
int ffm_engine_refresh_weights(ffm_engine *e, ffm_refresh_stats *out);
int ffm_group_refresh_weights(ffm_group *g, ffm_refresh_stats *out);

/* ---- Serving engines: FFM_FLAG_SERVE_F32 / FFM_FLAG_SERVE_F16 -----------------------------------------
 * predict() reads the stored w and nothing else (ffm.cpp:51-70), but a training engine's latent record is
 * [n][z][w]: scoring a saved model holds three times the bytes it reads.  With one of these flags
 * ffm_engine_create makes an engine that stores the bias (1 float), lin_w[n_feats] (fp32) and a latent table
 * [n_feats][n_fields * n_factors] of w ALONE -- no n or z anywhere, linear part included -- in
 *   FFM_FLAG_SERVE_F32   the training engine's fp32 bits: a third of the memory, bit-identical predictions;
 *   FFM_FLAG_SERVE_F16   IEEE binary16: a sixth of the memory, half the bytes per prediction.
 * LIMITS  FFM only, one whole model on one device (n_shards == 1, not inside ffm_group_create), n_factors in
 *         {4, 8, 16, 32, 64}: anything else is FFM_E_UNSUPPORTED.  Rows of at most 128 entries: max_row_nnz == 0
 *         means 128 here, a larger value is FFM_E_INVALID -- a serving engine has no kernel for longer rows (a
 *         longer host row is FFM_E_CAPACITY before anything is queued; a longer device row voids its block as
 *         usual: NaN outputs, FFM_E_CAPACITY at the next sync).  No training.  field_start is accepted and
 *         used for FFM_FLAG_HASH_IDS's per-field ranges only.
 * fp16    the contract: w -> binary16 by round to nearest even, subnormals kept, finite values beyond the
 *         half range to +-inf, NaN stays NaN (payload unspecified) -- numpy's astype(float16); decoding is the
 *         exact half -> float conversion.  A prediction is, bit for bit, the fp32 arithmetic of
 *         ffm_engine_predict_batch on the DECODED weights, in the same order.  The linear weights stay fp32.
 * create  every element is what a training engine of the same config would draw
 *         (ffm_engine_init_weights_host: same seed and index), rounded to the format; FFM_FLAG_SKIP_INIT gives
 *         zero bits.  So a sparse checkpoint -- a delta to a fresh engine -- means on a serving engine what it
 *         means on a training engine: set_rows its ids' lin_w / vec_w, set_weights its bias.
 * works   every prediction entry point, unchanged: ffm_engine_predict_batch, _device, _async, _async_scores
 *         (zero_copy included), ffm_engine_predict_finish_device; FFM_METRIC_EVAL; FFM_FLAG_HASH_IDS and
 *         ffm_engine_hash_ids_device; field == NULL and val == NULL rows; ffm_engine_sync, the profile calls (the predict
 *         kernel's label is "serve_wave_kernel"), ffm_engine_train_flush as the evaluation flush.
 *         ffm_engine_set_weights / set_rows take fp32 host arrays as always (w is rounded to the format on the
 *         device); ffm_engine_get_weights / get_rows return the decoded fp32 values.
 * refused with FFM_E_UNSUPPORTED ("a serving engine holds no accumulators"): every training entry point
 *         (synchronous, device, staged, pipelined, weighted, forward / update), ffm_engine_prepare_device,
 *         ffm_engine_set_state / get_state with any non-NULL pointer, set_rows / get_rows with a non-NULL n or
 *         z pointer, ffm_engine_changed_features, ffm_engine_refresh_weights, ffm_engine_fill_state.
 * A training engine is unchanged by all this: the same bytes, kernels and launches. */

/* src's stored bias, lin_w and the w component of every latent record into dst, in one streaming pass on the
 * device (no host copy of the model).  dst: a serving engine; src: an unsharded FFM training engine of the
 * same (n_feats, n_fields, n_factors) on the same device; anything else is FFM_E_INVALID.  It copies the
 * STORED w -- one update behind the accumulators ("Refresh" above): call ffm_engine_refresh_weights(src)
 * first when the learned model is wanted.  src is drained first as ffm_engine_refresh_weights drains it and
 * is not written; synchronous.  Counters (all but n_latent are 0 for FFM_FLAG_SERVE_F32):
 *   n_latent   latent elements written;
 *   n_inexact  elements whose decoded value differs in bits from the source (NaN to NaN does not count);
 *   n_to_inf   finite elements that became infinite;   n_to_zero  nonzero elements that became +-0.
 * out may be NULL.  The counter buffer (256 bytes of HBM) is allocated by dst's first call. */
typedef struct { int64_t n_latent, n_inexact, n_to_inf, n_to_zero; } ffm_pack_stats;
int ffm_engine_pack_weights(ffm_engine *dst, ffm_engine *src, ffm_pack_stats *out);

/* Bytes of HBM requested for the model arrays (bias, linear, latent) of any engine: an unsharded FFM
 * training engine 12 + 12 * n_feats + 12 * n_feats * row_len, a serving engine 4 + 4 * n_feats +
 * B * n_feats * row_len with B = 4 (fp32) or 2 (fp16); a shard counts the records it stores. */
int64_t ffm_engine_model_bytes(const ffm_engine *e);

/* ---- Scoring candidates: one context against many candidates, on a serving engine ----------------------
 * A REQUEST is a list of context entries (field, feat, val); each of its CANDIDATES is a list of entries.  The
 * score of a candidate is, bit for bit, what ffm_engine_predict_batch on the same engine returns for the
 * spelled-out row [context entries ..., candidate entries ...] -- logits and probabilities -- that is
 * FFM::predict (ffm.cpp:51-55) on that row:
 *   erasure  an id outside [0, n_feats) or a field outside [0, n_fields) is erased, in the context and in the
 *            candidate; the survivors keep their order;
 *   linear   summed sequentially from the bias: the context's survivors first, then the candidate's;
 *   pairs    each term is (dot * xa) * xb with the factor-order dot; the terms are summed one dependent add
 *            after another in the reference's pair order (a outer, b inner) over the concatenated survivors.
 * ROW ORDER  A caller whose rows are in field order, with the candidate fields after the context fields, gets
 *   the reference's bits.  Any other split gets the same terms added in the order of the concatenation.
 * What is shared between the candidates of a request, without giving up a bit: the running value after the
 * bias and the context's linear terms (a candidate continues from it), and the TERM of every context x context
 * pair -- computed once per request, stored, and fed by every candidate's wave into the same sequential sum at
 * the position the pair has in the concatenated row (the sum itself cannot be cut in two: in pair order those
 * terms interleave with the context x candidate ones).  The context's entries cross the link once per request,
 * and its pairs' latent slots are gathered once per request instead of once per candidate.
 *   Arrays: ctx_ptr[n_req + 1] delimits the requests' entries in ctx_field / ctx_feat / ctx_val;
 * cand_req_ptr[n_req + 1]: the candidates of request r are rows [cand_req_ptr[r], cand_req_ptr[r + 1]) of the
 * candidate block cand_ptr[n_cand + 1], cand_field / cand_feat / cand_val; a request may have none.
 * out[n_cand].  Candidates carry no labels: no loss is computed and the metrics channels are not fed.
 * LIMITS  The raw length of a row (context entries + candidate entries, before erasure) obeys the engine's
 *   max_row_nnz, at most 128; n_cand at most max_batch_rows, the candidates' entries at most max_batch_nnz.
 * ffm_engine_score_candidates: arrays in host memory; synchronous, like ffm_engine_predict_batch.  A deferred
 *   evaluation block is launched first.  Checked on the caller's thread before anything is queued: a null array
 *   or a pointer array that does not start at 0 or decreases, or cand_req_ptr[n_req] != n_cand: FFM_E_INVALID;
 *   n_cand > max_batch_rows, or a context + candidate longer than max_row_nnz: FFM_E_CAPACITY (out untouched).
 *   ctx_val == NULL / cand_val == NULL: every value is 1.0f.  On an engine with FFM_FLAG_HASH_IDS both id
 *   arrays are hashed on the device behind their copies.
 * ffm_engine_score_candidates_device: the same arrays in device memory (values required, ids taken as they
 *   are); ctx_nnz / cand_nnz: their entry counts; ctx_cap: the longest context of the call (raw); asynchronous
 *   on the engine's stream.  A request whose context is longer than ctx_cap or max_row_nnz has all of its
 *   candidates NaN; a candidate whose row is longer than max_row_nnz is NaN alone; either is reported as
 *   FFM_E_CAPACITY by ffm_engine_check_errors / ffm_engine_sync, as for ffm_engine_predict_batch_device.
 * Both: a training engine is refused with FFM_E_UNSUPPORTED (ffm_engine_pack_weights makes a serving engine
 *   from it); n_req == 0 or n_cand == 0 is FFM_OK with nothing written.  The per-request buffers (survivors,
 *   prefix, n_req * ctx_cap * (ctx_cap - 1) / 2 stored terms) are allocated at the first call, grown to the
 *   largest call seen and freed by ffm_engine_destroy; a failed allocation is FFM_E_NOMEM and leaves the engine
 *   usable.  The profile calls label the kernels "serve_context_kernel" and "serve_candidate_kernel".
 * OUT OF SCOPE  the CLI (there is no request file format to mirror); groups, shards, FM and LR; training
 *   engines; a pipelined or zero-copy variant; rows beyond 128 entries. */
int ffm_engine_score_candidates(ffm_engine *e, int32_t n_req, const int32_t *ctx_ptr, const int32_t *ctx_field,
                                const int32_t *ctx_feat, const float *ctx_val, const int32_t *cand_req_ptr,
                                int32_t n_cand, const int32_t *cand_ptr, const int32_t *cand_field,
                                const int32_t *cand_feat, const float *cand_val, int32_t output_prob, float *out);
int ffm_engine_score_candidates_device(ffm_engine *e, int32_t n_req, const int32_t *ctx_ptr, const int32_t *ctx_field,
                                       const int32_t *ctx_feat, const float *ctx_val, const int32_t *cand_req_ptr,
                                       int32_t n_cand, const int32_t *cand_ptr, const int32_t *cand_field,
                                       const int32_t *cand_feat, const float *cand_val, int32_t ctx_nnz,
                                       int32_t cand_nnz, int32_t ctx_cap, int32_t output_prob, float *out);

/* ---- Field ablation: the loss and AUC of the model without each field, in one pass -------------------
 * Which fields earn their place?  The standard answer is the evaluation loss and AUC of the same model with
 * field f removed from every row -- n_fields more passes over rewritten copies of the evaluation data.  The
 * wave kernels already stage everything those answers need: a row's surviving entries and every pair term,
 * added in the reference's order.  The logit of the row without field v is the same ordered sum with the terms
 * that touch v left out, and x + -0.0f == x, so it is exact.  The gathers and the k-long dots -- the cost of a
 * prediction -- are made once per row; what is new per variant is one dependent add per term.
 * DEFINITION  For a block and a field v in [0, n_fields), drop(block, v) is the block without every entry whose
 *   field is v; rows, labels and the order of the remaining entries stay as they are.
 *   variant v         of a row is ffm_engine_predict_batch of drop(block, v) at that row: the logit, the
 *                     probability and the logloss term, bit for bit, on this engine's stored weights.
 *   variant n_fields  is the row itself: ffm_engine_predict_batch of the block.
 *   erased entries    (an id or field out of range, negative) are erased before ablation, as always.
 *   a row without field v  has variant v equal to variant n_fields, bit for bit.
 *   multi-valued fields    every entry of the field goes.
 * ffm_engine_ablation_enable  allocates the (n_fields + 1) x max_batch_rows score and loss scratch and, with
 *   with_auc, n_fields + 1 score histograms of 16 MiB each (640 MiB at 39 fields), zeroed; a later call
 *   allocates only what is missing, and with_auc on it means what it means for ffm_engine_pair_ablation_enable
 *   (1 keeps what is collected, 0 stops the collection, a later 1 starts from zero).  The call is all or nothing:
 *   everything it has to make is made before anything of the engine changes, so a failed allocation is
 *   FFM_E_NOMEM, gives back what the call had made and leaves state and memory as they were (field ablation
 *   stays off, or on without histograms).  FFM_FIELD_HIST_FAIL=1 in the environment (and FFM_PAIR_HIST_FAIL=1
 *   for the pairs), a test hook read at each call, fails the histograms' allocation that way without filling a
 *   device.  All of it is freed by ffm_engine_destroy.  Refused with FFM_E_UNSUPPORTED and a
 *   message that says why: anything but a whole FFM model on one device (LR, FM, n_shards > 1, a group's
 *   engine, compact storage); n_factors outside {4, 8, 16, 32, 64}; n_fields > 64 (one lane per variant means
 *   one wave).  Works on training engines and on FFM_FLAG_SERVE_F32 / _F16 serving engines.
 * ffm_engine_predict_ablated  rows in host memory, synchronous, staged like ffm_engine_predict_batch: val == NULL
 *   is 1.0f, an engine with FFM_FLAG_HASH_IDS hashes the ids first (fields are not touched by hashing),
 *   field == NULL is FFM_E_INVALID.  out[(n_fields + 1) * n_rows] is variant-major (variant v of row r at
 *   v * n_rows + r; logits, or probabilities with output_prob) and may be NULL; loss_sum_out[n_fields + 1], may
 *   be NULL, holds per variant the double ffm_engine_predict_batch(drop(block, v)) returns (0 without labels).
 *   Before ffm_engine_ablation_enable: FFM_E_INVALID.
 * ffm_engine_predict_ablated_device  the same on arrays in device memory (values and fields required, ids taken
 *   as they are; out and loss_sum_out device arrays or NULL); asynchronous on the engine's stream.
 * rows too long  a row longer than max_row_nnz, or than the 128 entries a wave stages, is NaN in every variant
 *   and reported as FFM_E_CAPACITY (by the host call itself, by ffm_engine_sync after the device call), as a
 *   serving engine's rows are: there is no second launch behind this one.
 * ffm_engine_ablation_read  out[n_fields + 1]: per variant the ffm_metrics of its histogram -- the definition
 *   of "Metrics": same bins, integer counters, one entry per labelled row of every ablated block since the
 *   enable or the last reset.  Without with_auc: FFM_E_INVALID.
 * The calls feed neither FFM_METRIC_EVAL nor FFM_METRIC_TRAIN, and neither keyed capture.  An engine that
 * never enables ablation allocates nothing, launches nothing and changes in nothing; no existing kernel, launch
 * or argument list changed, FFM_ENGINE_ABI_VERSION and ffm_engine_config are what they were.
 * OUT OF SCOPE  a pipelined or staged form; groups and shards.  (Field pairs: "Pair ablation" below.) */
int ffm_engine_ablation_enable(ffm_engine *e, int32_t with_auc);
int ffm_engine_predict_ablated(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr, const int32_t *field,
                               const int32_t *feat, const float *val, const int32_t *label, int32_t output_prob,
                               float *out /* [(n_fields + 1) * n_rows], variant-major, may be NULL */,
                               double *loss_sum_out /* [n_fields + 1], may be NULL */);
int ffm_engine_predict_ablated_device(ffm_engine *e, int32_t n_rows, int32_t nnz, const int32_t *row_ptr,
                                      const int32_t *field, const int32_t *feat, const float *val, const int32_t *label,
                                      int32_t output_prob, float *out, double *loss_sum_out);
int ffm_engine_ablation_read(ffm_engine *e, int32_t reset, ffm_metrics *out /* [n_fields + 1] */);

/* ---- Pair ablation: the loss and AUC of the model without each field pair, in one pass ---------------
 * Which interactions carry the model?  An FFM model is a set of field-pair interactions (39 fields: 741 cross
 * pairs and 39 diagonal ones); a field can matter only through its linear term and two or three partners.  The
 * answer by hand is one evaluation pass per pair, and no rewrite of the rows removes a pair.  Here the gathers
 * and the k-long dots are made once per row, as for field ablation, and every pair's variant is one more ordered
 * sum of the same terms.
 * DEFINITION  F = n_fields <= 64.  The variants are the unordered field pairs with the diagonal, V = F (F + 1) / 2
 *   (at most 2080), numbered for f <= g by
 *     pair_index(f, g) = f * F - f * (f - 1) / 2 + (g - f);
 *   variant V is the row itself.
 *   variant (f, g)    of a row is the prediction's ordered sum -- bias, the survivors' linear products, then the
 *                     pair terms in ffm_engine_predict_batch's pair order -- with every term whose two entries
 *                     have the fields {f, g} left out (f == g: the terms between two entries of field f).  Linear
 *                     terms are never left out.  Leaving a term out and adding -0.0f in its place are the same
 *                     bits.  Every term belongs to exactly one variant.
 *   variant V         is ffm_engine_predict_batch of the block, bit for bit.
 *   a row without an entry of f, or of g (f == g: with fewer than two of f)  has variant (f, g) equal to variant V.
 *   as weights        in a block where every feature id occurs under one field only, on a model whose bias is not
 *                     -0.0f, variant (f, g) is ffm_engine_predict_batch of the block on the same model with the
 *                     latent slot "towards field g" set to +0.0f for every id of field f: those terms become
 *                     +-0.0f, and a running sum that starts at a bias other than -0.0f is never -0.0f, so adding
 *                     them changes no bit (engine.py: drop_pair_weights; this is how the tests check it).
 * ffm_engine_pair_count / _pair_index / _pair_fields  the numbering, on the host (no device, no engine):
 *   pair_count(F) = V; pair_index takes f, g in either order; pair_fields is its inverse (*f <= *g).  n_fields
 *   outside [1, 64], a field outside [0, n_fields) or v outside [0, V) sets the last error; the two counting calls
 *   then return -1 and pair_fields FFM_E_INVALID.
 * ffm_engine_pair_ablation_enable  allocates the (V + 1) x max_batch_rows score (fp32) and loss (fp64) scratch --
 *   12 bytes per variant and row: 77 MB for 39 fields and 8192-row blocks -- and, with with_auc, V + 1 score
 *   histograms of 16.8 MB each, zeroed: 13 GB at 39 fields, 35 GB at 64.  A later call allocates only what is
 *   missing.  with_auc decides whether histograms are collected from then on: with_auc == 1 while they are
 *   collected keeps their counts; with_auc == 0 on a later call stops the collection (the memory stays, and
 *   ffm_engine_pair_ablation_read is FFM_E_INVALID again); a later with_auc == 1 starts from zero.  A failed
 *   allocation is FFM_E_NOMEM and leaves the engine as it was, in state and in memory: everything the call has to
 *   make is made before anything changes, and what it had made before the failure is given back (pair ablation
 *   stays off, or on without histograms).  All of it is freed by ffm_engine_destroy.  Refused with FFM_E_UNSUPPORTED and a message that
 *   says why: anything but a whole FFM model on one device (LR, FM, n_shards > 1, a group's engine, compact
 *   storage); n_factors outside {4, 8, 16, 32, 64}; n_fields > 64.  Works on training engines and on
 *   FFM_FLAG_SERVE_F32 / _F16 serving engines.
 * ffm_engine_predict_pair_ablated  rows in host memory, synchronous, staged like ffm_engine_predict_ablated (the
 *   same upload: val == NULL is 1.0f; hashed ids, the rare fold, buckets and FFM_FLAG_NORM_ROWS apply first;
 *   field == NULL is FFM_E_INVALID; n_rows > max_batch_rows is refused as always).  out[(V + 1) * n_rows] is
 *   variant-major (variant v of row r at v * n_rows + r; logits, or probabilities with output_prob) and may be
 *   NULL: the scores then stay in HBM and only the loss sums come back.  loss_sum_out[V + 1], may be NULL, holds
 *   per variant the double sum of the rows' logloss terms as ffm_engine_predict_batch sums them (0 without
 *   labels).  Before ffm_engine_pair_ablation_enable: FFM_E_INVALID.
 * ffm_engine_predict_pair_ablated_device  the same on arrays in device memory (values and fields required, ids
 *   taken as they are; out and loss_sum_out device arrays or NULL); asynchronous on the engine's stream.
 * rows too long  a row longer than max_row_nnz, or than the 128 entries a wave stages, is NaN in every variant
 *   and reported as FFM_E_CAPACITY, exactly as for field ablation.
 * ffm_engine_pair_ablation_read  out[V + 1]: per variant the ffm_metrics of its histogram, as
 *   ffm_engine_ablation_read.  Without with_auc: FFM_E_INVALID.
 * The calls feed neither FFM_METRIC_EVAL nor FFM_METRIC_TRAIN, neither keyed capture, and nothing of field
 * ablation.  An engine that never enables pair ablation allocates nothing, launches nothing and changes in
 * nothing; the section adds functions only: no struct, no existing kernel, launch or argument list changed, and
 * FFM_ENGINE_ABI_VERSION is what it was.
 * Acting on the answer -- predicting without the pairs that carry nothing -- is "Pair masks" below.
 * OUT OF SCOPE  pair variants of ffm_engine_score_candidates; groups, shards, LR and FM; a pipelined or staged
 *   form. */
int32_t ffm_engine_pair_count(int32_t n_fields);
int32_t ffm_engine_pair_index(int32_t n_fields, int32_t f, int32_t g);
int ffm_engine_pair_fields(int32_t n_fields, int32_t v, int32_t *f, int32_t *g);
int ffm_engine_pair_ablation_enable(ffm_engine *e, int32_t with_auc);
int ffm_engine_predict_pair_ablated(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr, const int32_t *field,
                                    const int32_t *feat, const float *val, const int32_t *label, int32_t output_prob,
                                    float *out /* [(V + 1) * n_rows], variant-major, may be NULL */,
                                    double *loss_sum_out /* [V + 1], may be NULL */);
int ffm_engine_predict_pair_ablated_device(ffm_engine *e, int32_t n_rows, int32_t nnz, const int32_t *row_ptr,
                                           const int32_t *field, const int32_t *feat, const float *val, const int32_t *label,
                                           int32_t output_prob, float *out, double *loss_sum_out);
int ffm_engine_pair_ablation_read(ffm_engine *e, int32_t reset, ffm_metrics *out /* [V + 1] */);

/* ---- Pair masks: predict with the kept field pairs only ----------------------------------------------------
 * Pair ablation says which pairs carry the model; a mask acts on it.  A prediction row is its pair gathers (39
 * fields: 741 pairs x two 64-byte slots), and under a mask the pairs left out are gathers not made: the masked
 * kernel's loads, dots and ordered-sum steps are those of the kept pairs.
 * DEFINITION  keep[n_fields], one uint64_t per field, n_fields <= 64.  Bit g of keep[f]: "the terms between an
 *   entry of field f and an entry of field g are part of the prediction".  The mask is symmetric (bit g of keep[f]
 *   equals bit f of keep[g]); bit f of keep[f] is the diagonal, two entries of one field; bits at or above
 *   n_fields are zero.  The masked prediction of a row is ffm_engine_predict_batch's ordered sum -- the bias, the
 *   survivors' linear products in row order, then the kept pair terms in predict_batch's pair order (a outer, b
 *   inner), every addition sequential -- with every pair term whose two surviving entries' fields (f, g) have the
 *   bit clear LEFT OUT (not added as zero).  Linear terms always stay.  remove_out_range, rows without values,
 *   hashed ids, the rare fold, buckets and FFM_FLAG_NORM_ROWS act exactly as they do without a mask, before it: the
 *   norm is not recomputed for the pairs that go.
 *   all bits set      is ffm_engine_predict_batch, bit for bit.
 *   one pair dropped  is variant (f, g) of "Pair ablation", bit for bit, on any block.
 *   as weights        under the two conditions of "Pair ablation" (one field per id in the block, a bias other than
 *                     -0.0f) it is predict_batch on the model with the slot towards g zeroed for field f's ids, for
 *                     every dropped pair (f, g) in both directions.
 * ffm_engine_set_pair_mask  keep == NULL clears the mask.  Otherwise the words are copied to the device, ordered on
 *   the engine's stream; a deferred evaluation block (ffm_engine_predict_batch_async) is launched first, as by every
 *   entry point that queues work, so blocks queued earlier are scored under the earlier mask and later ones under
 *   the new one.  Nothing of the caller's is read after the call returns.
 *   FFM_E_UNSUPPORTED, with a message that says why: LR and FM; n_shards > 1; a group's engine; compact storage;
 *   n_factors outside {4, 8, 16, 32, 64}; n_fields > 64; a training engine created with FFM_PREDICT_WAVE=0.
 *   FFM_E_INVALID, leaving the previous mask in force: n_fields other than the engine's; an asymmetric mask; a bit
 *   at or above n_fields; staged training blocks still waiting.
 * ffm_engine_get_pair_mask  *is_set is 1 or 0; keep_out[n_fields] (may be NULL) the words in force, zeros without.
 * WHERE IT APPLIES  every row-prediction entry point of an engine with a mask launches the masked kernel:
 *   ffm_engine_predict_batch, _predict_batch_device, _predict_batch_async[_scores] (zero_copy 0 and 1) and
 *   _predict_batch_async_resident, on training engines and on FFM_FLAG_SERVE_F32 / _F16 engines.  What they feed
 *   sees masked scores because it reads those outputs: the loss sums, FFM_METRIC_EVAL, keyed capture on the eval
 *   channel, streamed scores.
 * rows too long  a row longer than max_row_nnz, or than the 128 entries a wave stages, is NaN and reported as
 *   FFM_E_CAPACITY -- on a training engine too: a masked engine launches no other row kernel.
 * WHILE A MASK IS SET  FFM_E_INVALID, before anything is queued, model and state unchanged: every training entry
 *   point, ffm_engine_score_candidates[_device], ffm_engine_predict_ablated*, ffm_engine_predict_pair_ablated* and
 *   ffm_engine_predict_pair_curve*.
 *   Masked training and masked candidates are different features; refusing keeps anything from silently running
 *   unmasked.
 * The mask is not part of the model: weights and state in and out, ffm_engine_pack_weights, _sync_weights, deltas,
 * _refresh_weights and checkpoints neither read nor record it, exactly as they do not record field ranges.  An
 * engine that never sets a mask allocates nothing, launches the kernels it launched before with the arguments it
 * passed before; the section adds functions only, and FFM_ENGINE_ABI_VERSION is what it was.
 * OUT OF SCOPE  pruned or re-packed tables that drop the masked slots from memory; masks in
 *   ffm_engine_score_candidates and in the ablation kernels; training under a mask; groups, shards, LR and FM;
 *   recording the mask in checkpoints. */
int ffm_engine_set_pair_mask(ffm_engine *e, const uint64_t *keep /* [n_fields], NULL clears */, int32_t n_fields);
int ffm_engine_get_pair_mask(ffm_engine *e, uint64_t *keep_out /* [n_fields], may be NULL */, int32_t *is_set);

/* ---- Pruning curve: the loss and AUC of up to 64 pair masks, in one pass -----------------------------------
 * Pair ablation says what ONE pair is worth to the whole model; those deltas do not add up when hundreds of pairs go
 * together.  Where pruning starts to hurt is the curve "loss and AUC against kept pairs", and by hand every point of
 * it is one masked evaluation pass.  Here the gathers and the k-long dots are made once per row, as for the two
 * ablations, and every point is one more ordered sum of the same terms.
 * DEFINITION  A level table is level[n_fields][n_fields]: uint16_t, row-major with stride n_fields, symmetric, the
 *   diagonal included.  A list of n_cuts cuts goes with it, 1 <= n_cuts <= 64; each cut is an int32_t in [0, 65536],
 *   in any order, duplicates allowed.
 *   variant c         (c < n_cuts) of a row is the prediction's ordered sum -- the bias, the survivors' linear
 *                     products, then the pair terms in ffm_engine_predict_batch's pair order -- with the terms
 *                     between an entry of field f and an entry of field g left out wherever level[f][g] >= cut[c].
 *                     Linear terms always stay.  Leaving a term out and adding -0.0f in its place are the same bits.
 *   variant n_cuts    is ffm_engine_predict_batch of the block, bit for bit.
 *   as masks          variant c is, bit for bit, ffm_engine_predict_batch of the same block on the same engine under
 *                     ffm_engine_set_pair_mask(M_c), bit g of M_c[f] = (level[f][g] < cut[c]) -- on any block, with
 *                     no condition on the ids (engine.py: pair_curve_mask is this sentence in numpy).  Cut 0 keeps no
 *                     pair, cut 65536 keeps all.
 *   a ladder          with level = a pair's rank in an importance order (engine.py: pair_curve_levels), cut N is
 *                     "keep the best N pairs": nested masks.  The engine requires neither nesting nor ranks.
 * ffm_engine_pair_curve_enable  the engine restrictions and messages of the ablations (FFM_E_UNSUPPORTED: anything
 *   but a whole FFM model on one device; n_factors outside {4, 8, 16, 32, 64}; n_fields > 64).  FFM_E_INVALID,
 *   leaving what was in force: n_fields other than the engine's, an asymmetric table, n_cuts outside [1, 64], a cut
 *   outside [0, 65536].  Allocates the (n_cuts + 1) x max_batch_rows score and loss scratch and, with with_auc,
 *   n_cuts + 1 score histograms of 16.8 MB each, as ffm_engine_pair_ablation_enable does and with with_auc meaning
 *   what it means there.  The table and the cuts are copied to engine-owned device memory before the call returns,
 *   on the engine's stream and into arrays of their own: the kernels queued so far go on reading the previous ones.
 *   Calling it again replaces the table and the cuts; if n_cuts changed, the scratch is made again and the
 *   histograms start from zero.  With n_cuts unchanged the histograms KEEP their counts, as with_auc says, also when
 *   the table or the cuts are others: the counts then mix two ladders, so read them with reset = 1
 *   (ffm_engine_pair_curve_read) before changing the table.  A failed allocation is FFM_E_NOMEM, a failed copy
 *   FFM_E_DEVICE; either leaves the engine as it was (the curve off, or the previous table, cuts and counts in force).
 * ffm_engine_predict_pair_curve[_device]  the arguments, staging and errors of ffm_engine_predict_pair_ablated
 *   [_device]; out[(n_cuts + 1) * n_rows] variant-major, may be NULL; loss_sum_out[n_cuts + 1], may be NULL.
 *   Before ffm_engine_pair_curve_enable, and while a pair mask is set: FFM_E_INVALID.
 * rows too long  a row longer than max_row_nnz, or than the 128 entries a wave stages, is NaN in all n_cuts + 1
 *   variants and reported as FFM_E_CAPACITY.
 * ffm_engine_pair_curve_read  out[n_cuts + 1]: per variant the ffm_metrics of its histogram.  Without with_auc:
 *   FFM_E_INVALID.
 * The calls feed neither metric channel, no keyed capture and nothing of the two ablations.  An engine that never
 * enables the curve allocates nothing and launches nothing of it; the section adds functions only, and
 * FFM_ENGINE_ABI_VERSION is what it was.
 * OUT OF SCOPE  more than 64 cuts a pass (a second call with other cuts covers that); groups, shards, LR and FM;
 *   training under a mask. */
int ffm_engine_pair_curve_enable(ffm_engine *e, const uint16_t *level /* [n_fields * n_fields] */, int32_t n_fields,
                                 const int32_t *cut /* [n_cuts] */, int32_t n_cuts, int32_t with_auc);
int ffm_engine_predict_pair_curve(ffm_engine *e, int32_t n_rows, const int32_t *row_ptr, const int32_t *field,
                                  const int32_t *feat, const float *val, const int32_t *label, int32_t output_prob,
                                  float *out /* [(n_cuts + 1) * n_rows], variant-major, may be NULL */,
                                  double *loss_sum_out /* [n_cuts + 1], may be NULL */);
int ffm_engine_predict_pair_curve_device(ffm_engine *e, int32_t n_rows, int32_t nnz, const int32_t *row_ptr,
                                         const int32_t *field, const int32_t *feat, const float *val, const int32_t *label,
                                         int32_t output_prob, float *out, double *loss_sum_out);
int ffm_engine_pair_curve_read(ffm_engine *e, int32_t reset, ffm_metrics *out /* [n_cuts + 1] */);

/* ---- Serving deltas: sync a serving engine, publish only what moved --------------------------------------
 * ffm_engine_pack_weights takes all of a model: it streams every record of the training engine and writes the
 * whole table.  A trainer that never stops moves a few per cent of its features between two publications;
 * these entry points find those features, list them, and move their rows in the table's own bits.
 * ffm_engine_sync_weights  dst, src, the drains and the stream are those of ffm_engine_pack_weights, with the
 *   same checks and the same errors.  Per feature i:
 *   target    the linear pattern is the bits of src.lin_w[i]; the row is enc(src w[i][e]) for every e < row_len,
 *             enc the format's own encoding (the identity for fp32, the fp16 rule of "Serving engines").
 *   moved     i is MOVED iff its target linear pattern differs from the bits dst.lin_w[i] holds, or any target
 *             element differs from the bits stored in dst's row -- patterns, not values, in the table's own
 *             width: -0.0f against +0.0f is moved; a NaN whose encoded bits are the stored ones is not; an fp32
 *             change that rounds to the same half is not moved on an fp16 engine.
 *   dst       afterwards dst's bias, lin_w and table are, bit for bit, what ffm_engine_pack_weights(dst, src)
 *             would have left; a feature that is not moved is not written.
 *   stats     n_moved: the moved features; n_lin_moved, n_lat_moved: the elements whose patterns differed;
 *             bias_moved: 0 or 1 (the bias is in no list).  out may be NULL.
 *   bitmap    the moved set of the LAST call stays in dst as a bitmap in HBM, ceil(n_feats / 64) 64-bit words,
 *             allocated (with 256 bytes of counters) by dst's first call and freed by ffm_engine_destroy; each
 *             call overwrites it.
 *   ordering  everything runs on dst's stream: predictions queued before the call see the old weights, those
 *             queued after it the new ones.  Synchronous, like ffm_engine_pack_weights.
 * ffm_engine_sync_moved  the bitmap as ascending ids, with the argument conventions of
 *   ffm_engine_changed_features: ids == NULL counts; a cap below the count is FFM_E_CAPACITY with *n_moved set;
 *   before any ffm_engine_sync_weights on this engine: FFM_E_INVALID.
 * ffm_engine_get_rows_raw / set_rows_raw  the listed features' lin_w (fp32) and rows as the table stores them:
 *   lat is [n][row_len] elements of 4 bytes (FFM_FLAG_SERVE_F32) or 2 (FFM_FLAG_SERVE_F16), no conversion in
 *   either direction -- an fp16 engine's delta is half the bytes and keeps NaN payloads.  Either array may be
 *   NULL.  Serving engines only: a training engine is FFM_E_UNSUPPORTED; an id outside [0, n_feats) is
 *   FFM_E_INVALID before anything is moved, as for ffm_engine_get_rows / set_rows.  Synchronous.
 * An engine that never calls these allocates nothing and launches nothing; no existing kernel, launch or
 * argument list changed, FFM_ENGINE_ABI_VERSION and ffm_engine_config are what they were.
 * OUT OF SCOPE  groups and shards, LR / FM; deltas between two training engines. */
typedef struct { int64_t n_moved, n_lin_moved, n_lat_moved, bias_moved; } ffm_sync_stats;
int ffm_engine_sync_weights(ffm_engine *dst, ffm_engine *src, ffm_sync_stats *out);
int ffm_engine_sync_moved(ffm_engine *dst, int32_t *ids, int64_t cap, int64_t *n_moved);
int ffm_engine_get_rows_raw(ffm_engine *e, int32_t n, const int32_t *ids, float *lin_w,
                            void *lat /* [n][row_len] of 2 or 4 bytes */);
int ffm_engine_set_rows_raw(ffm_engine *e, int32_t n, const int32_t *ids, const float *lin_w, const void *lat);

/* ---- Text blocks: libffm / libsvm text parsed on the device ------------------------------------------------
 * Every row enters as text, and a libffm row of 39 entries is about as many bytes of text as of field / feat / val.
 * A text parser takes the BYTES of whole lines and leaves, in HBM, the CSR block the host parser (parse_csr_range,
 * host/csr_reader.cpp) would have produced for them: row_ptr [n_rows + 1], label [n_rows], field / feat / val [nnz],
 * as every _device entry point and every *_add_device takes them.  It needs no engine.
 *   grammar    the host parser's fast path and nothing else, stated rule by rule in csrc/text_parse.h ("Text
 *              blocks"), which host and device share bit for bit: lines end at '\n' or the text's end, one trailing
 *              '\r' is stripped, the only blank is ' ', a line of blanks is no row; the label is [+-] and 1 to 9
 *              digits (1 if > 0, else 0); an entry is field:feat:value (has_field) or feat:value (field = 0) with ids
 *              of 1 to 9 digits and a value [-]digits[.digits] of at most 7 significant and 10 fraction digits,
 *              float(digits) / 10^n_frac in one correctly rounded division; an entry that compares equal to 0.0f is
 *              dropped.
 *   slow       every other line -- an exponent, nan, inf, a tab, a '+' on a value, a missing part, a 10-digit id, a
 *              label such as 1.0, more than FFM_TEXT_MAX_LINE bytes before the '\n'.  A slow line is not parsed and
 *              nothing is guessed: it counts in n_slow, gives no row and no entry, and the caller hands the text to
 *              the host parser.
 *   block      n_lines (lines of the text, an unterminated last one included), n_rows and nnz (of the lines that
 *              are not slow: TRUE totals, also when they exceed the capacities), n_slow, first_slow_byte (offset of
 *              the first slow line's first byte, -1 without one) and overflow (n_rows > max_rows or nnz > max_nnz)
 *              are always valid; the arrays only when n_slow == 0 and overflow == 0.  The pointers are DEVICE
 *              pointers into the slot, valid until the slot's next parse.
 *   slots      two: _parse (asynchronous, on the parser's own stream) copies and parses chunk t + 1 while the
 *              caller consumes chunk t; _wait is the one host wait per chunk (the consumers take nnz from the host).
 *              zero_copy != 0: text is page-locked (ffm_engine_pin_host) and stays untouched until _wait on that
 *              slot returns; otherwise the parser copies it into a page-locked image of its own first, and text is
 *              free when _parse returns.  Whoever reads a slot's arrays on another stream has them read before the
 *              slot is parsed into again.
 *   refused    FFM_E_INVALID: n_bytes > max_bytes or negative, a slot outside {0, 1}, _parse on a slot whose last
 *              parse was not waited for, _wait on a slot nothing was parsed into, max_bytes outside [1, 2^31 - 4096],
 *              a capacity below 1; FFM_E_DEVICE without a device.
 *   host       ffm_engine_textparse_host is the same grammar on the host, bit for bit, and needs no device: it
 *              fills the caller's arrays (row_ptr [max_rows + 1], label [max_rows], field / feat / val [max_nnz])
 *              under the same rule and stores nothing past them; the block's pointers come back NULL.
 * OUT OF SCOPE  parsing the slow grammar on the device; a fallback per line (a block falls back whole). */
typedef struct ffm_textparse ffm_textparse;
#define FFM_TEXT_MAX_LINE 65536
typedef struct {
  int64_t n_lines, n_rows, nnz;       /* true totals, also on overflow                  */
  int64_t n_slow, first_slow_byte;    /* slow lines; offset of the first one's first byte */
  int32_t overflow;                   /* n_rows > max_rows or nnz > max_nnz: arrays not valid */
  const int32_t *row_ptr, *field, *feat, *label;  /* DEVICE pointers, valid until the slot's next parse */
  const float *val;
} ffm_text_block;
int ffm_engine_textparse_create(int32_t has_field, int64_t max_bytes, int32_t max_rows, int32_t max_nnz, int32_t device_id,
                                ffm_textparse **out);
int ffm_engine_textparse_parse(ffm_textparse *p, int32_t slot /* 0 or 1 */, const char *text, int64_t n_bytes,
                               int32_t zero_copy); /* asynchronous */
int ffm_engine_textparse_wait(ffm_textparse *p, int32_t slot, ffm_text_block *out);
void ffm_engine_textparse_destroy(ffm_textparse *p);
int ffm_engine_textparse_host(int32_t has_field, const char *text, int64_t n_bytes, int32_t max_rows, int32_t max_nnz,
                              int32_t *row_ptr, int32_t *field, int32_t *feat, float *val, int32_t *label, ffm_text_block *out);

/* ---- Resident rows: blocks cut out of parsed text in HBM, staged without crossing PCIe again ------------------
 * A text parser leaves a chunk's rows in HBM in the layout the engine wants.  A ROW CUTTER cuts them into the blocks
 * a trainer would have cut -- so many rows, so many entries at the most, across chunk borders -- without the host
 * touching an entry, and the three staged entry points have twins that take such a block.  Everything behind the
 * source of the bytes is shared with the host forms: the same upload kernel instantiations (hashing, rare-id folding,
 * bucketing), the same row normalisation, grouping, schedule and numbering (ffm_engine_blocks_pulled / _scored), so
 * every result is the host form's bit for bit.
 *   mirror     ffm_engine_textparse_wait_rows is ffm_engine_textparse_wait and also hands back a page-locked HOST
 *              mirror of the slot's row_ptr [n_rows + 1] -- all the host needs of a chunk to place the cuts.  NULL
 *              when the block's arrays are not valid (n_slow != 0 or overflow).  It is valid until the slot's next
 *              parse.  The first such wait allocates the mirrors (4 bytes per row of max_rows, both slots) and
 *              copies its own behind the parse; from then on every parse copies its slot's on the parser's stream
 *              ahead of the slot's event, and the wait stays the one host wait per chunk.  A parser that never asks
 *              allocates and copies nothing.
 *   cutter     ffm_engine_rowcut_create: a ring of n_blocks (1 .. 64) buffers in HBM, each row_ptr [max_rows + 1],
 *              label [max_rows], field / feat / val [max_nnz], 16-byte aligned.  It needs no engine.
 *   take       appends rows [r0, r1) of the block waited for in `slot` (with _wait_rows) to the block being
 *              assembled: ONE kernel launch on the PARSER's stream -- so the slot's arrays are read before the slot
 *              is parsed into again, by stream order -- copies the entries and labels, 16 bytes per lane where the
 *              alignments allow, and rebases row_ptr to the block's running entry count (row_ptr[0] of a block is
 *              0).  The launch is sized by the host from the mirror; the kernel reads no count from memory, and every
 *              store is guarded by the buffer's capacity.  Asynchronous.
 *   take_host  the same for rows the HOST parsed (a chunk the device will not parse: ffm_text_block.n_slow,
 *              overflow, a line longer than a slot): row_ptr [n_rows + 1] may start at any value, field / feat / val
 *              point at entry row_ptr[0] and label at the first row.  It appends at the same position, so device-
 *              and host-parsed rows may meet in one block.  The arrays are free when it returns.
 *   close      ends the block: its n_rows, nnz and longest row (all known on the host), the DEVICE pointers, `index`
 *              (its buffer) and `ready`, an event behind the block's last take.  A block of no rows is valid.  The
 *              ring moves on.
 *   release    the buffer `index` may be written again.  The caller releases a block once the engine has pulled it:
 *              the resident entry points store the block's staging number in ffm_rows_block.seq, and the block is
 *              free when ffm_engine_blocks_pulled has reached it -- the rule of page-locked blocks.  Until then a
 *              take or close into that buffer is FFM_E_CAPACITY, and nothing is launched.
 *   staging    ffm_engine_stage_batch_resident / _train_batch_async_resident / _predict_batch_async_resident are
 *              ffm_engine_stage_batch / _train_batch_async_pinned (three blocks in flight) /
 *              _predict_batch_async_scores (scores_host may be NULL) with zero_copy != 0, for a block whose arrays
 *              are DEVICE memory of the engine's device, 16-byte aligned: the upload waits for `ready` (may be NULL:
 *              the block is whole) on the engine's side stream and reads HBM.  Any such block will do, a cutter's or
 *              the caller's own.  field is ignored on LR / FM; FFM needs it, and every block brings val.
 *   refused    what the host forms refuse, with their codes and texts: n_rows > max_batch_rows and nnz >
 *              max_batch_nnz (FFM_E_CAPACITY), longest_row > max_row_nnz (FFM_E_CAPACITY), training on a serving
 *              engine (FFM_E_UNSUPPORTED), a missing array; longest_row outside [0, nnz] and an array that is not
 *              16-byte aligned are FFM_E_INVALID.  longest_row is trusted beyond that, as nnz is on every _device
 *              entry point.  A take beyond max_rows / max_nnz of the cutter is FFM_E_CAPACITY before anything is
 *              launched; rows outside the slot's block, a slot that was not waited for with _wait_rows, a parser on
 *              another device are FFM_E_INVALID.
 * An engine that never calls these allocates nothing and launches nothing new; no existing kernel changed.
 * OUT OF SCOPE  sample weights on this path; offline mode (whole files shuffled on the host); groups and shards;
 *               copying chunk t + 1 on a second stream while chunk t parses; any change to the text kernels; a
 *               fallback per line (a chunk falls back whole). */
typedef struct ffm_rowcut ffm_rowcut;
typedef struct {
  int32_t n_rows, nnz, longest_row;  /* longest_row: the most entries of one row (0 in a block without entries) */
  int32_t index;                     /* the cutter's buffer (ffm_engine_rowcut_release); unused by the engine */
  int64_t seq;                       /* OUT of the resident entry points: the block's staging number */
  const int32_t *row_ptr, *field, *feat, *label;  /* DEVICE pointers, 16-byte aligned */
  const float *val;
  void *ready;                       /* hipEvent_t behind the block's last write, or NULL */
} ffm_rows_block;
int ffm_engine_textparse_wait_rows(ffm_textparse *p, int32_t slot, ffm_text_block *out, const int32_t **row_ptr_host);
int ffm_engine_rowcut_create(int32_t max_rows, int32_t max_nnz, int32_t n_blocks, int32_t device_id, ffm_rowcut **out);
int ffm_engine_rowcut_take(ffm_rowcut *c, ffm_textparse *p, int32_t slot, int32_t r0, int32_t r1); /* asynchronous */
int ffm_engine_rowcut_take_host(ffm_rowcut *c, int32_t n_rows, const int32_t *row_ptr, const int32_t *field,
                                const int32_t *feat, const float *val, const int32_t *label);
int ffm_engine_rowcut_close(ffm_rowcut *c, ffm_rows_block *out);
int ffm_engine_rowcut_release(ffm_rowcut *c, int32_t index);
void ffm_engine_rowcut_destroy(ffm_rowcut *c);
int ffm_engine_stage_batch_resident(ffm_engine *e, ffm_rows_block *block);
int ffm_engine_train_batch_async_resident(ffm_engine *e, ffm_rows_block *block);
int ffm_engine_predict_batch_async_resident(ffm_engine *e, ffm_rows_block *block, int32_t output_prob,
                                            float *scores_host);

#ifdef __cplusplus
}
#endif
#endif /* FFM_ENGINE_H */
