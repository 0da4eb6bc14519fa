// engine.hip -- host side of the C ABI in include/ffm_engine.h: owns the model state in HBM and the
// per-block scratch, and schedules the gfx950 kernels of one block of rows on one HIP stream.
//
// Pipeline of one training block (DESIGN.md "Pipeline"):
//   group_keys -> radix sort (rocPRIM) -> group_finish              (kernels_group.h)
//   ffm_refresh           lazy refresh, once per distinct feature   (kernels_row.h)
//   {ffm,fm}_row<TRAIN>   lazy refresh + forward -> logit           (kernels_row.h)
//   [cross-shard sum of the logits when n_shards > 1 -- done by the caller, RCCL]
//   tmp_grad -> loss_sum
//   the (n, z) update of every touched accumulator, folded by        (kernels_fold.h, kernels_update.h,
//   reductions: bias, linear, {ffm,fm} latent                         kernels_tile.h)
// There is no CPU fallback anywhere in this library.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include <algorithm>
#include <cmath>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <optional>
#include <mutex>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/ffm_engine.h"
#include "engine_types.h"
#include "init_rng.h"
#include "hash_ids.h"
#include "kernels_group.h"
#include "kernels_row.h"
#include "kernels_fold.h"
#include "kernels_update.h"
#include "kernels_tile.h"
#include "kernels_fm.h"
#include "kernels_wave.h"
#include "kernels_sort.h"
#include "kernels_scan.h"
#include "kernels_refresh.h"
#include "kernels_metric.h"
#include "kernels_keyed.h"
#include "kernels_serve.h"
#include "kernels_delta.h"
#include "kernels_ablate.h"
#include "kernels_ablate_pairs.h"
#include "kernels_curve.h"
#include "kernels_mask.h"
#include "kernels_stage.h"
#include "kernels_sketch.h"
#include "kernels_idcount.h"
#include "kernels_valhist.h"
#include "kernels_norm.h"
#include "kernels_text.h"
#include "kernels_rows.h"
#include "metrics_host.h"

using namespace ftrl_dev;

// The grouping's sort: always the Onesweep radix sort (a few passes over the key bits), never
// rocPRIM's merge-sort variant (about twenty small launches at this size).
// (Its default tuning -- 1024-thread workgroups, twenty of them for a block -- only finds room when a
// kernel beside it drains; 256-thread configurations do find room and were measured slower for the
// step: the sort then takes wave slots from the kernels on the critical path.)
using GroupSortConfig = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                                  rocprim::default_config, 0>;

namespace {

thread_local std::string g_last_error;

// FFM_HOST_TIMING=1: wall time the submitting thread spends in labelled sections (debug aid)
struct HostTimers {
  bool on = std::getenv("FFM_HOST_TIMING") != nullptr;
  struct Acc { const char *name; double total = 0, worst = 0; long n = 0; } acc[16];
  int n_acc = 0;
  Acc &get(const char *name) {
    for (int i = 0; i < n_acc; i++) if (acc[i].name == name) return acc[i];
    acc[n_acc].name = name;
    return acc[n_acc < 15 ? n_acc++ : 15];
  }
  ~HostTimers() {
    if (!on) return;
    for (int i = 0; i < n_acc; i++)
      std::fprintf(stderr, "[host timing] %-22s n=%6ld total=%9.3f ms mean=%8.1f us worst=%9.1f us\n",
                   acc[i].name, acc[i].n, acc[i].total * 1e3, acc[i].total * 1e6 / std::max(1l, acc[i].n), acc[i].worst * 1e6);
  }
} g_timers;
struct ScopedTimer {
  const char *name;
  std::chrono::steady_clock::time_point t0;
  explicit ScopedTimer(const char *n) : name(n) { if (g_timers.on) t0 = std::chrono::steady_clock::now(); }
  ~ScopedTimer() {
    if (!g_timers.on) return;
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    static std::mutex mu;  // (the staging thread times its sections too)
    std::lock_guard<std::mutex> lock(mu);
    auto &a = g_timers.get(name);
    a.total += s; a.n++; if (s > a.worst) a.worst = s;
  }
};

int fail(int code, const std::string &msg) {
  g_last_error = msg;
  return code;
}

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t err__ = (expr);                                                              \
    if (err__ != hipSuccess)                                                                \
      return fail(err__ == hipErrorOutOfMemory ? FFM_E_NOMEM : FFM_E_DEVICE,                \
                  std::string(#expr) + ": " + hipGetErrorString(err__));                    \
  } while (0)

enum KernelId {
  K_GROUP_KEYS, K_GROUP_SORT, K_GROUP_FINISH, K_ROW, K_TMP_GRAD,
  K_LOSS_SUM, K_LINEAR_UPDATE, K_BIAS_UPDATE, K_LATENT_UPDATE, K_LATENT_UPDATE_FEW, K_LATENT_UPDATE_WALK, K_LATENT_UPDATE_GIANT,
  K_PREDICT_ROW, K_REFRESH, K_LATENT_UPDATE_SINGLE, K_METRIC, K_PUSH_SCORES, K_SERVE_ROW,
  K_SERVE_CTX, K_SERVE_CAND,
  K_KEYED_CAPTURE, K_KEYED_SORT_HIST, K_KEYED_SORT_SCAN, K_KEYED_SORT_SCATTER, K_KEYED_RANK,
  K_UPLOAD, K_NORM_ROWS,
  K_COUNT
};
const char *kKernelNames[K_COUNT] = {
    "group_keys_kernel", "group_radix_sort", "group_finish_kernel", "row_kernel<train>", "tmp_grad_kernel", "loss_sum_kernel",
    "linear_update_kernel", "bias_update_kernel", "update_kernel", "update_few_kernel", "update_walk_kernel", "update_giant_kernel",
    "row_kernel<predict>", "refresh_kernel", "update_single_kernel", "metric_hist_kernel", "push_scores_kernel", "serve_wave_kernel",
    "serve_context_kernel", "serve_candidate_kernel",
    "keyed_capture_kernel", "keyed_sort_hist_kernel", "keyed_sort_scan_kernels", "keyed_sort_scatter_kernel", "keyed_rank_kernels",
    "pull_block_kernel", "normalize_rows_kernel"};

struct ProfRec {
  int kid;
  hipEvent_t e0, e1;
};

// Where element e of the LOGICAL latent row of feature `feat` ([n_fields][n_factors] for FFM, the
// reference's layout, ffm.cpp:138-146) lives: a pointer to component `comp` of it, or null when
// this shard does not store it (compact storage keeps only the owned slots of the kept fields).
__device__ __forceinline__ float *logical_elem(const ModelDev &m, int64_t feat, int e, int comp) {
  if (!m.field_start)
    return m.lat + feat * 3 * m.row_len + static_cast<int64_t>(comp) * m.row_len + e;
  int lo = 0, hi = m.n_fields;  // field of the id: field_start[fa] <= feat < field_start[fa + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (m.field_start[mid] <= feat) lo = mid; else hi = mid;
  }
  const int fa = lo, fp = e / m.n_factors, kk = e - fp * m.n_factors;
  const int sl = fp - m.own_lo[fa];
  if (static_cast<unsigned>(sl) >= static_cast<unsigned>(m.own_n[fa])) return nullptr;
  return lat_row(m, static_cast<int>(feat), fa) + static_cast<int64_t>(comp) * m.row_len + sl * m.n_factors + kk;
}

// `logical_len` = n_fields * n_factors (FFM) or n_factors (FM): every draw is addressed by its
// logical coordinates, so a shard initialises its slots to the values the unsharded model holds.
__global__ void init_weights_kernel(ModelDev m, int logical_len, float mean, float stddev, uint64_t seed) {
  const int64_t n_lat = static_cast<int64_t>(m.n_feats) * logical_len;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; idx < n_lat;
       idx += stride) {
    const int64_t feat = idx / logical_len;
    float *p = logical_elem(m, feat, static_cast<int>(idx - feat * logical_len), LAT_W);
    if (p) *p = ftrl_rng::init_weight(seed, 1, idx, mean, stddev);
  }
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < m.n_feats;
       i += stride)
    m.lin_w[i] = ftrl_rng::init_weight(seed, 0, i, mean, stddev);
}

__global__ void fill_state_kernel(ModelDev m, int logical_len, uint64_t seed, float n_lo, float n_hi, float z_sd) {
  const int64_t n_lat = static_cast<int64_t>(m.n_feats) * logical_len;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  const int64_t t0 = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  auto unif = [&](uint64_t stream, int64_t idx) {
    return n_lo + (n_hi - n_lo) * ftrl_rng::uniform01(seed, stream, idx);
  };
  auto normal01 = [](uint64_t sd, uint64_t stream, int64_t idx) { return ftrl_rng::normal01(sd, stream, idx); };
  for (int64_t idx = t0; idx < n_lat; idx += stride) {
    const int64_t feat = idx / logical_len;
    const int e = static_cast<int>(idx - feat * logical_len);
    float *pn = logical_elem(m, feat, e, LAT_N);
    if (!pn) continue;
    *pn = unif(11, idx);
    pn[m.row_len] = z_sd * normal01(seed, 12, idx);  // the z row follows the n row
  }
  for (int64_t i = t0; i < m.n_feats; i += stride) {
    m.lin_n[i] = unif(13, i);
    m.lin_z[i] = z_sd * normal01(seed, 14, i);
  }
  if (t0 == 0) {
    m.bias3[1] = unif(15, 0);
    m.bias3[2] = z_sd * normal01(seed, 16, 0);
  }
}

// Proves div_alpha_fast == IEEE divide for this alpha over every float significand, both signs
// and two exponents (ftrl_math.h); any mismatch raises *bad.
__global__ void verify_div_alpha_kernel(Hyper h, int *bad) {
  const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;  // 2^25 threads
  const unsigned mant = idx & 0x7fffffu;
  const unsigned expo = (idx >> 23) & 1u ? 0x3f800000u : 0x40000000u;
  const unsigned sign = (idx >> 24) & 1u ? 0x80000000u : 0u;
  const float x = __uint_as_float(sign | expo | mant);
  const float a = div_alpha_fast(h, x), b = x / h.alpha;
  if (__float_as_uint(a) != __float_as_uint(b)) atomicOr(bad, 1);
}

// Compares sqrt_fast / sqrt_fast0 (ftrl_math.h) with sqrtf on EVERY float of their range,
// [2^-96, 2^96] and +0, on the device the engine runs on; any mismatch raises *bad.
__global__ void verify_sqrt_fast_kernel(int *bad) {
  const unsigned lo = __float_as_uint(0x1p-96f), hi = __float_as_uint(0x1p96f);
  const unsigned stride = gridDim.x * blockDim.x;
  bool differs = false;
  for (unsigned b = lo + blockIdx.x * blockDim.x + threadIdx.x; b <= hi && b >= lo; b += stride) {
    const float x = __uint_as_float(b);
    const unsigned want = __float_as_uint(sqrtf(x));
    differs = differs || __float_as_uint(sqrt_fast(x)) != want || __float_as_uint(sqrt_fast0(x)) != want;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) differs = differs || __float_as_uint(sqrt_fast0(0.0f)) != 0u;
  if (differs) atomicOr(bad, 1);
}

// Copies one component (n, z or w) of features [feat0, feat0+nf) between the stored records and a
// dense [feat][logical_len] staging buffer (the reference's save order).  Slots this shard does
// not store read as 0 and ignore writes.
__global__ void lat_component_copy_kernel(ModelDev m, int logical_len, int comp, float *dense,
                                          int64_t feat0, int64_t nf, int to_dense) {
  const int64_t total = nf * logical_len;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; idx < total;
       idx += stride) {
    const int64_t f = idx / logical_len;
    float *p = logical_elem(m, feat0 + f, static_cast<int>(idx - f * logical_len), comp);
    if (to_dense) dense[idx] = p ? *p : 0.0f; else if (p) *p = dense[idx];
  }
}

// The same for a list of features: component `comp` of ids[j] <-> dense[j][logical_len]
// (ffm_engine_get_rows / set_rows).
__global__ void lat_rows_copy_kernel(ModelDev m, int logical_len, int comp, float *dense,
                                     const int *ids, int64_t nf, int to_dense) {
  const int64_t total = nf * logical_len;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; idx < total;
       idx += stride) {
    const int64_t j = idx / logical_len;
    const int i = ids[j];
    float *p = (i < 0 || i >= m.n_feats) ? nullptr
                                          : logical_elem(m, i, static_cast<int>(idx - j * logical_len), comp);
    if (to_dense) dense[idx] = p ? *p : 0.0f; else if (p) *p = dense[idx];
  }
}
__global__ void lin_rows_copy_kernel(float *lin, int n_feats, float *dense, const int *ids, int nf,
                                     int to_dense) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nf) return;
  const int i = ids[j];
  if (i < 0 || i >= n_feats) { if (to_dense) dense[j] = 0.0f; return; }
  if (to_dense) dense[j] = lin[i]; else lin[i] = dense[j];
}

#include "engine_plan.h"
#include "engine_select.h"
}  // namespace

struct ffm_engine {
  ffm_engine_config cfg{};
  ModelDev m{};
  // kSets sets of grouping outputs, used in rotation: block t+1 is grouped on the prep stream into
  // the set block t-2 used, so it never waits for block t-1 or t to retire (with two sets the
  // grouping could only start when the previous block ended, and then sat starved of wave slots
  // behind that block's persistent update kernels).  What the row kernel writes is shared.
  static constexpr int kSets = 4;
  Scratch sc[kSets]{};
  int cur = 0;                 // set of the block being trained
  bool cur_prepared = false;   // ... was grouped ahead (ev_grouped[cur] marks the end of its grouping)
  int *h_super = nullptr;      // [kSets] page-locked: Scratch::n_super of every set, as the host reads it
  // evaluation block whose predict launch ffm_engine_predict_batch_async deferred by one call
  // (scores: where its predictions go in the caller's page-locked memory, as the device sees it, or
  // null; seq: its staging number, which push_scores_kernel publishes)
  struct {
    bool on = false; int slot = 0; bool labelled = false;
    float *scores = nullptr; int output_prob = 0; int64_t seq = 0;
  } eval_pending;
  bool eval_defer_off = false;  // FFM_EVAL_DEFER=0
  bool super_wait = true;       // wait for a block's grouping before deciding on its super launches (FFM_SUPER_WAIT=0: only ask)
  bool super_flag_ok = false;  // create proved that a device store to h_super reaches the host
  // groupings made ahead by ffm_engine_prepare_device, oldest first (at most kSets - 1)
  int n_prepared = 0;
  int prepared_set[kSets] = {};
  Rows prepared_rows[kSets] = {};
  int last_set = 0;            // set handed out most recently (to a prepare or to a training block)
  bool set_used[kSets] = {};
  hipStream_t prep = nullptr;  // side stream of ffm_engine_prepare_device
  // Uploads of staged host blocks (pull_block_kernel) go on the prep stream, ahead of the block's
  // grouping.  (A fifth stream for them shares a hardware queue with one of the four and
  // serialises with it: measured 1.45-1.70 ms per step instead of 1.3.)
  bool pull_after_row = false;  // a staged block's upload waits for the running block's row kernel to end (long steps)
  bool own_sort = false;        // the grouping's sort: kernels_sort.h (short steps) or rocPRIM Onesweep (engine_create.h: choose_sort)
  bool range_sort = false;      // ... or, when the id ranges of the fields are known, a workgroup per range (kernels_sort.h)
  int *d_sort_start = nullptr;  // [n_sort_ranges + 1] the ranges' boundaries, the last one = n_feats
  int n_sort_ranges = 0;
  int sort_grid_cap = 1;        // workgroups of the one-launch sort the device holds at once (its grid barrier needs them all)
  hipEvent_t ev_grouped[kSets] = {}, ev_set_free[kSets] = {};
  hipEvent_t ev_row_done[kSets] = {};  // the row kernel of the block trained from the set has ended
  bool prep_after_row = false;         // a look-ahead grouping starts beside an UPDATE phase (FFM_PREP_AFTER_ROW)
  // Scheduling of a look-ahead grouping: the block being
  // prepared will start training when its predecessor's update ends; its grouping is made to
  // START when the block before that one ends -- so it runs beside the predecessor's refresh and
  // row phases (memory-bound, ~400 us, the grouping takes ~300 us there) and never beside an
  // update phase, where the update's kernels starve it (a Onesweep pass then takes 250-300 us
  // instead of 7) and it slows them.  trained_set[0] / [1]: the scratch sets of the
  // training blocks enqueued last / before that (their ev_set_free marks the end of the update).
  int trained_set[2] = {-1, -1};
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // Streams: the runtime multiplexes streams onto few hardware queues (4 by default), and two
  // streams on one queue run one after the other -- so no more than stream + 2 side + prep here.
  hipStream_t aux3 = nullptr;  // side stream: a shard's once-only / few-occurrence launches beside its update
                               // launch; the few-occurrence launch of a side-by-side update
  hipEvent_t ev_fork = nullptr, ev_fork2 = nullptr, ev_join = nullptr, ev_join2 = nullptr;
  hipStream_t aux4 = nullptr;  // second side stream of the update (FFM_UPDATE_SPLIT=2)
  int max_rows = 0, max_nnz = 0, max_row_nnz = 1024;
  // staging for the host-buffer entry points
  int *d_row_ptr = nullptr, *d_field = nullptr, *d_feat = nullptr, *d_label = nullptr;
  float *d_val = nullptr, *d_out = nullptr;
  float *d_weight = nullptr;  // [max_rows] sample weights of a ffm_engine_train_batch_weighted block (allocated by the first)
  double *d_loss_sum = nullptr;
  // pipelined host-buffer training (ffm_engine_train_batch_async): kSlots staging slots, each a
  // pinned host image and device arrays of one block; block t is copied + grouped on the prep
  // stream while block t-1 trains on the main stream and the caller builds block t+1
  static constexpr int kSlots = 4;
  struct Slot {
    char *pinned = nullptr;
    int *row_ptr = nullptr, *field = nullptr, *feat = nullptr, *label = nullptr;
    float *val = nullptr;
    hipEvent_t ev_copied = nullptr, ev_trained = nullptr;
    // what frees the slot's device arrays: the scratch set's ev_set_free of the block that trained from
    // it (no record of its own: one packet less on the main stream per step), ev_trained after a prediction
    hipEvent_t free_ev = nullptr;
    bool used = false, zero_copy = false;
    int64_t seq = 0;  // 1-based number of the block staged in it
    int n_rows = 0, nnz = 0, row_cap = 0;
    bool has_field = false;
    // sample weights of the block (ffm_engine_stage_batch_weighted): the device array and its pinned
    // image, both allocated when the engine first stages a weighted block; valid, like the labels, until
    // the slot is refilled -- after its block's update
    float *weight = nullptr;
    char *pinned_w = nullptr;
    bool has_weight = false;
  } slots[kSlots];
  bool slot_weights_ready = false;
  bool slots_ready = false;
  int slot_next = 0;
  int staged[kSlots] = {};  // slots staged and not yet in training, oldest first
  int n_staged = 0;
  int cur_slot = -1;        // slot of the block between train_forward_staged and train_update
  int64_t n_staged_total = 0, n_pulled = 0;  // blocks staged so far / known to be uploaded
  // The upload kernel of block number b (1-based; uploads run in staging order) writes b into a
  // word of page-locked host memory when its last workgroup is done: ffm_engine_blocks_pulled is a
  // plain read.  (Per staging slot would not do -- a slot is refilled, on the HOST's timeline, while
  // the GPU may still be several blocks behind --, and an event per block costs the submitting
  // thread a query per poll and the runtime a signal per block.)
  long long *h_pulled = nullptr;       // hipHostMalloc
  long long *d_pulled = nullptr;       // the same word as the device sees it
  unsigned *d_pull_ticket = nullptr;   // workgroups of the running upload kernel that are done
  // The same for the scores going the other way (ffm_engine_predict_batch_async_scores): the
  // download kernel of a scored block writes the block's staging number into a word of its own.
  long long *h_scored = nullptr;       // hipHostMalloc
  long long *d_scored = nullptr;       // the same word as the device sees it
  unsigned *d_score_ticket = nullptr;  // workgroups of the running download kernel that are done
  int64_t n_scored = 0;                // the largest number read from h_scored so far
  double *d_loss_acc = nullptr;  // [1] sum of the async blocks' losses since the last flush
  double *d_loss_part = nullptr; // [kLossParts + 1] loss_sum_kernel's partial sums and ticket
  void *d_sort_tmp[kSets] = {};  // rocPRIM radix sort workspace per scratch set
  size_t sort_tmp_bytes = 0;
  unsigned sort_bits = 32;
  float *d_stage = nullptr;  // dense staging for get/set
  int64_t stage_floats = 0;
  int *d_ids = nullptr;      // feature ids of one ffm_engine_get_rows / set_rows chunk
  static constexpr int kIdsCap = 1 << 20;
  int *d_err = nullptr;      // [1] sticky ERR_* flags of every block since the last report
  // the AUC channels (include/ffm_engine.h "Metrics"): hist = pos[kMetricBins], neg[kMetricBins], n_nan;
  // allocated when the channel is first turned on
  struct MetricChannel { bool on = false; unsigned long long *hist = nullptr; } metric[2];
  // keyed capture (include/ffm_engine.h "Metrics", engine_keyed.h): per channel the captured words and the four
  // counters of kernels_keyed.h; shared by both, since reads run one after another on the stream: the sort's
  // scratch buffer and histogram, the scans' tile sums, the per-key table.  All made by ffm_engine_metrics_key_field.
  struct KeyedChannel {
    bool on = false;
    unsigned long long *words = nullptr, *counters = nullptr;
    size_t words_cap = 0;
  } keyed[2];
  int keyed_field = -1;
  int64_t keyed_capacity = 0;  // rows a channel stores at the most (the buffers may be larger)
  unsigned long long *keyed_scratch = nullptr, *keyed_tab = nullptr;
  unsigned *keyed_hist = nullptr, *keyed_hist_sums = nullptr, *keyed_n_keys = nullptr;
  ftrl_dev::RankState *keyed_rank_sums = nullptr;
  int *keyed_tab_key = nullptr;
  size_t keyed_scratch_cap = 0, keyed_tab_cap = 0, keyed_tab_key_cap = 0, keyed_rank_sums_cap = 0;
  bool in_group = false;  // made by ffm_group_create
  // FFM_FLAG_HASH_IDS (engine_hash.h): host rows have their ids hashed on the device before any kernel reads
  // them; hm.start = the device copy of field_start (FFM with per-field id ranges) or null = [0, n_feats)
  bool hash_ids = false;
  ftrl_hash::Map hm{};
  int *d_hash_start = nullptr;
  // ffm_engine_set_rare_fold (engine_idcount.h): the keep-map in HBM (its own allocation, freed when the fold is
  // turned off or the engine destroyed) and its shift; words == nullptr: no fold, and nothing here is read
  ftrl_hash::Rare rare{};
  // ffm_engine_set_buckets (engine_valhist.h): the bucket table in HBM (one allocation of its own, n_edges first, freed
  // when the table is taken off or the engine destroyed); n_edges == nullptr: none, and nothing here is read
  ftrl_hash::Buckets buckets{};
  // FFM_FLAG_NORM_ROWS (engine_norm.h): every row of a host block is scaled to unit length on the device behind its
  // upload and id rewriting.  d_norm_unscaled: [1] rows the kernel left as they came (made at create on a flagged
  // engine, else by the first ffm_engine_normalize_rows_device); norm_rows: rows it was launched on (the staging
  // thread counts too); grid_norm: its workgroups at the most, a run of 64 rows each (FFM_GRID_NORM)
  bool norm_rows_on = false;
  unsigned long long *d_norm_unscaled = nullptr;
  std::atomic<int64_t> norm_rows{0};
  int grid_norm = 1024;
  // ffm_engine_refresh_weights (engine_refresh.h): its six counters and its grid, both made by the first call
  unsigned long long *d_refresh = nullptr;
  int refresh_grid = 0;
  // ffm_engine_pack_weights (engine_serve.h): the four counters of a serving engine, made by the first call
  unsigned long long *d_pack = nullptr;
  // ffm_engine_sync_weights (engine_delta.h), both made by a serving engine's first call: its four counters, and
  // the features the LAST call moved as a bitmap of ceil(n_feats / 64) words
  unsigned long long *d_sync = nullptr, *d_moved = nullptr;
  bool synced = false;
  // ffm_engine_score_candidates[_device] (engine_serve.h): what serve_context_kernel leaves for the candidates'
  // waves (cx) and the host call's staging of the context arrays, made by the first call, grown to the largest
  // call seen; the capacities in elements
  ftrl_dev::CandCtx cx{};
  int *d_ctx_ptr = nullptr, *d_req_ptr = nullptr, *d_ctx_field = nullptr, *d_ctx_feat = nullptr;
  float *d_ctx_val = nullptr;
  size_t cx_ent_cap = 0, cx_head_cap = 0, cx_terms_cap = 0, cx_cand_cap = 0;
  size_t ctx_ptr_cap = 0, req_ptr_cap = 0, ctx_field_cap = 0, ctx_feat_cap = 0, ctx_val_cap = 0;
  // field and pair ablation (include/ffm_engine.h "Field ablation", "Pair ablation"; engine_ablate.h), each set all
  // made by its enable call for its V variants -- n_fields + 1, or n_fields (n_fields + 1) / 2 + 1 --: out [V][max_rows]
  // scores and loss the same shape (the kernel's variant-major outputs), sums [V], part [V][kLossParts + 1] the loss
  // sums' partial sums and tickets, hist [V][2 * kMetricBins + 1] with with_auc
  struct AblateSet {
    bool on = false, auc = false;
    int variants = 0;  // V of the arrays below (the curve's changes with its cuts: its set is then made again)
    float *out = nullptr;
    double *loss = nullptr, *sums = nullptr, *part = nullptr;
    unsigned long long *hist = nullptr;
  } abl, pabl, cabl;
  // the pruning curve (include/ffm_engine.h "Pruning curve"; engine_ablate.h): cabl above for its n_cuts + 1 variants,
  // and the level table and cuts in force in HBM, made by the first ffm_engine_pair_curve_enable
  unsigned short *d_curve_level = nullptr;  // [kCurveFields * kCurveFields], the first n_fields * n_fields in use
  int *d_curve_cut = nullptr;               // [kCurveCuts], the first cabl.variants - 1 in use
  // ffm_engine_set_pair_mask (include/ffm_engine.h "Pair masks", engine_mask.h): the words in HBM (made by the first
  // call that sets a mask) and their copy on the host; pair_mask_on == false: no mask, and nothing here is read
  bool pair_mask_on = false;
  unsigned long long *d_pair_mask = nullptr;  // [kMaskFields]
  uint64_t pair_mask[ftrl_dev::kMaskFields] = {};
  std::vector<void *> allocs;
  // split-phase bookkeeping
  Rows pending{};
  const float *pending_weight = nullptr;  // sample weights of the pending block (device) or null
  bool has_pending = false;
  // train_batch_device on one shard: the row kernel has the whole logit, so it also produces
  // tmp_grad and the row losses (no tmp_grad pass)
  bool own_tg_cur = false;
  // the block's lazy refresh as one pass over its distinct features (ffm_refresh_kernel) instead
  // of per occurrence inside the row kernel; FFM_ENGINE_ROW_REFRESH=1 keeps it in the row kernel
  bool pre_refresh = false;
  // 1: every distinct feature in ffm_refresh_kernel; 2: the once-only ones by their row; 3: and
  // updated there too when the row kernel has the whole logit (FFM_ENGINE_ROW_REFRESH=0/2/3)
  int refresh_mode = 3;
  bool singles_in_row = false;  // the block in flight had its once-only features updated by the row kernel
  unsigned long long *d_ownmask = nullptr;
  bool lin_any = true;          // this shard owns the linear terms of at least one field
  int logical_len = 0;          // n_fields * n_factors (FFM), n_factors (FM), 0 (LR): the reference's row
  int64_t n_records = 0;        // stored latent records (n_feats, or fewer on a compact shard)
  std::vector<int> field_start; // copy of cfg->field_start (compact shards)
  // workgroups of the update launch's ranges: few-occurrence features, hot tiles, the row-order walk
  // of serial slots; and of the once-only kernel of a shard
  int grid_small = 768, grid_hot = 2048, grid_walk = 256, grid_single = 768, grid_giant = 1024;
  int update_split = -1;  // FFM_UPDATE_SPLIT: 0 the update's ranges as ONE launch; 2 as three launches side by side
                          // on three queues (hot + bias + linear | few + serial walk + loss | giant), each with the
                          // registers and LDS of its own path; 1 as launches one after another (timing aid);
                          // default: 2 for a whole model's large launches (nnz * k >= 4 M: the fork / join pays), else 0
  int wide_max_nnz = 100000;  // FFM_WIDE_NNZ: blocks below this many entries run the update launch with eight-wave workgroups (0: never)
  bool predict_waves = true;  // FFM_PREDICT_WAVE=0: evaluation rows through ffm_row_kernel (one workgroup per row)
  int update_order = 210;     // FFM_UPDATE_ORDER: the update launch's big ranges, first range = last digit (0 giant, 1 hot, 2 few)
  // workgroups of pull_block_kernel.  Few on purpose: its loads take microseconds
  // (PCIe) and every one in flight holds a miss entry of an L2; 128 workgroups (512 KB in flight)
  // slowed the HBM-bound kernels they ran beside up to 4x (refresh of a 65536-row block 70 -> 330 us),
  // 24 (96 KB, about the link's bandwidth-delay product) still move the block at link rate.
  int grid_pull = 24;
  // workgroups of push_scores_kernel (FFM_GRID_PUSH, at most the upload's 24): one 16-byte store per
  // lane moves an 8192-row block with 8 (profiles/score_cost.md)
  int grid_push = 8;
  int row_threads = kRowThreads;  // workgroup size of the FFM row kernel (FFM_ROW_THREADS)
  int row_park = -1;         // FFM_ROW_PARK: bytes of w the row kernel parks in LDS (-1: what the budget leaves)
  int row_park_budget = 0;   // FFM_ROW_PARK_BUDGET: the row kernel's LDS budget for parking (0: 24 KB)
  int row_hold = -1;         // FFM_ROW_HOLD: (n, z) vectors per thread the row kernel holds in registers (-1: chosen by the launcher, 0: none)
  bool serial = false;  // FFM_ENGINE_SERIAL=1: no side streams (per-kernel timings without overlap)
  // ---- staging thread ------------------------------------------------------------------------
  // The GPU submissions of a staged block (its upload kernel and the ~10 launches of its grouping,
  // all on the prep stream) are issued by a thread of the engine's own, two blocks ahead of the
  // training launches that the caller's thread issues.  Why: rocPRIM's radix sort calls
  // hipMemsetAsync inside, which on this runtime can hold the submitting thread until earlier work
  // of the stream has retired -- measured 30 us per sort call on most boxes of the pool but 240 us
  // mean / 31 ms worst on others (profiles/archive/r03_host_leg_diag.txt), during which the caller's thread
  // did not enqueue the NEXT training block and the H2D-inclusive step grew from 1.13 to 1.32 ms
  // with the resident step unchanged.  All bookkeeping stays on the caller's thread; the worker only
  // replays closures in order.  staged_issued: ordinal of the last staged block whose launches are
  // out (a training call waits for ITS block only, never for the look-ahead's).
  std::thread worker;
  std::mutex wmu;
  std::condition_variable wcv_job, wcv_done;
  std::deque<std::function<int()>> wjobs;
  bool wstop = false, wbusy = false;
  int64_t staged_issued = 0;
  int worker_rc = 0;
  std::string worker_msg;
  void worker_main() {
    (void)hipSetDevice(cfg.device_id);
    for (;;) {
      std::function<int()> job;
      {
        std::unique_lock<std::mutex> lock(wmu);
        wcv_job.wait(lock, [&] { return wstop || !wjobs.empty(); });
        if (wjobs.empty()) return;
        job = std::move(wjobs.front());
        wjobs.pop_front();
        wbusy = true;
      }
      const int rc = job();
      {
        std::lock_guard<std::mutex> lock(wmu);
        if (rc != 0 && worker_rc == 0) { worker_rc = rc; worker_msg = g_last_error; }
        wbusy = false;
      }
      wcv_done.notify_all();
    }
  }
  // Runs `job` on the staging thread (or right here while kernels are being timed).
  int submit(std::function<int()> job) {
    if (prof_on) return job();
    {
      std::lock_guard<std::mutex> lock(wmu);
      if (!worker.joinable()) worker = std::thread([this] { worker_main(); });
      wjobs.push_back(std::move(job));
    }
    wcv_job.notify_one();
    return 0;
  }
  int worker_error() {  // an error of an earlier deferred submission surfaces at the next wait
    if (worker_rc == 0) return 0;
    const int rc = worker_rc;
    worker_rc = 0;
    return fail(rc, "staging thread: " + worker_msg);
  }
  // Until everything submitted so far is issued (before the caller's thread touches the prep stream).
  int drain() {
    std::unique_lock<std::mutex> lock(wmu);
    wcv_done.wait(lock, [&] { return wjobs.empty() && !wbusy; });
    return worker_error();
  }
  // Until the launches of staged block number `seq` are issued.
  int wait_issued(int64_t seq) {
    std::unique_lock<std::mutex> lock(wmu);
    wcv_done.wait(lock, [&] { return staged_issued >= seq || (wjobs.empty() && !wbusy); });
    return worker_error();
  }
  void stop_worker() {
    {
      std::lock_guard<std::mutex> lock(wmu);
      wstop = true;
    }
    wcv_job.notify_all();
    if (worker.joinable()) worker.join();
  }
  // profiling
  bool prof_on = false;
  int prof_only = -1;  // >= 0: record only this kernel id (ffm_engine_profile_focus)
  std::vector<ProfRec> prof;
  std::vector<hipEvent_t> event_pool;

  template <typename T>
  int alloc(T **p, size_t count) {
    void *q = nullptr;
    if (count == 0) count = 1;
    hipError_t err = hipMalloc(&q, count * sizeof(T));
    if (err != hipSuccess)
      return fail(FFM_E_NOMEM, "hipMalloc of " + std::to_string(count * sizeof(T)) +
                                   " bytes failed: " + hipGetErrorString(err));
    allocs.push_back(q);
    *p = static_cast<T *>(q);
    return FFM_OK;
  }
  // *p holds at least `need` elements afterwards.  The new array is made before the old one is let go, so a
  // failed allocation (FFM_E_NOMEM) leaves the engine as it was; hipFree waits for what still reads the old one.
  template <typename T>
  int grow(T **p, size_t *cap, size_t need) {
    if (*p && *cap >= need) return FFM_OK;
    T *q = nullptr;
    if (int rc = alloc(&q, need)) return rc;
    release(p);
    *p = q;
    *cap = need;
    return FFM_OK;
  }
  // An array alloc made, given back; *p is null afterwards.
  template <typename T>
  void release(T **p) {
    if (!*p) return;
    allocs.erase(std::find(allocs.begin(), allocs.end(), static_cast<void *>(*p)));
    (void)hipFree(*p);
    *p = nullptr;
  }

  hipEvent_t get_event() {
    if (!event_pool.empty()) {
      hipEvent_t e = event_pool.back();
      event_pool.pop_back();
      return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
  }
  void prof_begin(int kid, hipStream_t st) {
    prof_skip = !prof_on || (prof_only >= 0 && kid != prof_only);
    if (prof_skip) return;
    ProfRec r{kid, get_event(), get_event()};
    if (!r.e0 || !r.e1) {  // out of events: this launch goes untimed
      if (r.e0) event_pool.push_back(r.e0);
      if (r.e1) event_pool.push_back(r.e1);
      prof_skip = true;
      return;
    }
    (void)hipEventRecord(r.e0, st);
    prof.push_back(r);
  }
  bool prof_skip = true;
  void prof_end(hipStream_t st) {
    if (prof_skip) return;
    (void)hipEventRecord(prof.back().e1, st);
  }
};

// A serving engine (FFM_FLAG_SERVE_F32 / _F16, engine_serve.h) stores w alone: whatever needs (n, z) is refused.
static inline bool serving(const ffm_engine *e) { return e->m.lat_fmt != SERVE_NONE; }
static int serve_refuse(const char *what) {
  return fail(FFM_E_UNSUPPORTED, std::string("a serving engine holds no accumulators: ") + what + " needs a training engine");
}
#define SERVE_REFUSE(e, what) do { if ((e) && serving(e)) return serve_refuse(what); } while (0)
// An engine with a pair mask (engine_mask.h) predicts rows and nothing else: whatever would run unmasked is refused.
static int mask_refuse(const char *what) {
  return fail(FFM_E_INVALID, std::string(what) + " is not available while a pair mask is set (ffm_engine_set_pair_mask "
                                                 "with keep == NULL clears it): it would run without the mask");
}
#define MASK_REFUSE(e, what) do { if ((e) && (e)->pair_mask_on) return mask_refuse(what); } while (0)

#define LAUNCH_ON(e, st, kid, kernel, grid, block, shmem, ...)                   \
  do {                                                                           \
    (e)->prof_begin(kid, st);                                                    \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), shmem, st, __VA_ARGS__); \
    (e)->prof_end(st);                                                           \
  } while (0)
#define LAUNCH(e, kid, kernel, grid, block, shmem, ...) \
  LAUNCH_ON(e, (e)->stream, kid, kernel, grid, block, shmem, __VA_ARGS__)

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline int loss_grid(int n_rows) { return std::max(1, std::min(kLossParts, cdiv(n_rows, 1024))); }

// The update launch (kernels_tile.h) is instantiated per number of facts a stager lane of the hot
// features' tiles carries: slots per 64-element chunk / 4.
static int tile_nf(const ffm_engine *e) {
  const int k = e->m.n_factors, spc = k <= 64 ? 64 / k : 1;
  return spc > 8 ? 4 : spc > 4 ? 2 : 1;
}
// The once-only / few-occurrence kernels over a flat (feature, vector) index space instead of a
// wave per feature: when a wave per feature would leave more than a sixth of its lanes idle on a
// compact shard's records (40 vectors at 8 shards, 80 at 2 or 4).  For full-length records (156
// vectors, 81 % lane use) the flat shape measured no better.
static bool flat_pays(const ffm_engine *e, int span4) {
  if (e->m.n_shards <= 1 || span4 <= 0) return false;
  const int lanes = (span4 + 63) / 64 * 64;
  return span4 * 6 < lanes * 5;
}

#include "engine_count.h"

extern "C" {

int ffm_engine_abi_version(void) { return FFM_ENGINE_ABI_VERSION; }
int ffm_engine_block_segment(void) { return ftrl_dev::kSeg; }
const char *ffm_engine_last_error(void) { return g_last_error.c_str(); }

void ffm_engine_default_config(ffm_engine_config *cfg) {
  if (!cfg) return;
  std::memset(cfg, 0, sizeof(*cfg));
  cfg->model_type = FFM_MODEL_FFM;  // cmd_option.h:62
  cfg->n_feats = 10000;
  cfg->n_fields = 8;
  cfg->n_factors = 16;
  cfg->w_alpha = 1e-4f;
  cfg->w_beta = 1.0f;
  cfg->w_l1 = 0.1f;
  cfg->w_l2 = 5.0f;
  cfg->init_mean = 0.0f;
  cfg->init_stddev = 0.02f;
  cfg->seed = 42;
  cfg->max_batch_rows = 8192;
  cfg->max_batch_nnz = 8192 * 64;
  cfg->device_id = 0;
  cfg->n_shards = 1;
  cfg->shard_rank = 0;
}

int64_t ffm_engine_row_len(const ffm_engine *e) { return e ? e->logical_len : 0; }

void ffm_engine_destroy(ffm_engine *e) {
  if (!e) return;
  (void)hipSetDevice(e->cfg.device_id);
  e->stop_worker();  // (issues what is still queued, then joins)
  // everything the engine has in flight -- uploads still reading the caller's page-locked arrays
  // (staged, never trained), look-ahead groupings, the side streams -- ends before anything is freed
  if (e->prep) (void)hipStreamSynchronize(e->prep);
  if (e->aux3) (void)hipStreamSynchronize(e->aux3);
  if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
  if (e->ev_fork2) (void)hipEventDestroy(e->ev_fork2);
  if (e->ev_join) (void)hipEventDestroy(e->ev_join);
  if (e->ev_join2) (void)hipEventDestroy(e->ev_join2);
  if (e->aux4) (void)hipStreamDestroy(e->aux4);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  for (auto &r : e->prof) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  for (auto ev : e->event_pool) (void)hipEventDestroy(ev);
  for (auto &sl : e->slots) {
    if (sl.pinned) (void)hipHostFree(sl.pinned);
    if (sl.pinned_w) (void)hipHostFree(sl.pinned_w);
    if (sl.ev_copied) (void)hipEventDestroy(sl.ev_copied);
    if (sl.ev_trained) (void)hipEventDestroy(sl.ev_trained);
  }
  for (void *p : e->allocs) (void)hipFree(p);
  if (e->rare.words) (void)hipFree(const_cast<uint64_t *>(e->rare.words));
  if (e->buckets.n_edges) (void)hipFree(const_cast<int32_t *>(e->buckets.n_edges));
  for (int i = 0; i < ffm_engine::kSets; i++) {
    if (e->ev_grouped[i]) (void)hipEventDestroy(e->ev_grouped[i]);
    if (e->ev_set_free[i]) (void)hipEventDestroy(e->ev_set_free[i]);
    if (e->ev_row_done[i]) (void)hipEventDestroy(e->ev_row_done[i]);
  }
  if (e->h_pulled) (void)hipHostFree(e->h_pulled);
  if (e->h_scored) (void)hipHostFree(e->h_scored);
  if (e->h_super) (void)hipHostFree(e->h_super);
  if (e->prep) (void)hipStreamDestroy(e->prep);

  if (e->aux3) (void)hipStreamDestroy(e->aux3);
  if (e->own_stream && e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
}

#include "engine_create.h"

// What init_weights_kernel stored, computed on the host (csrc/init_rng.h: same bits).
static int eval_launch_pending(ffm_engine *e);  // (engine_stage.h)
// (engine_serve.h: the packed table <-> host arrays, for get / set_weights and get / set_rows)
static int serve_vec_transfer(ffm_engine *e, float *host, bool to_host);
static int serve_rows_vec_transfer(ffm_engine *e, int nf, float *host, bool to_host);

int ffm_engine_init_weights_host(uint64_t seed, float init_mean, float init_stddev, int32_t latent,
                                 int64_t first, int64_t count, float *out) {
  if (first < 0 || count < 0 || (count > 0 && !out)) return fail(FFM_E_INVALID, "bad range or null output");
  for (int64_t j = 0; j < count; j++)
    out[j] = ftrl_rng::init_weight(seed, latent ? 1 : 0, static_cast<uint64_t>(first + j), init_mean, init_stddev);
  return FFM_OK;
}

int ffm_engine_fill_state(ffm_engine *e, uint64_t seed, float n_lo, float n_hi, float z_stddev) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  SERVE_REFUSE(e, "ffm_engine_fill_state");
  if (!(n_lo >= 0.0f) || !(n_hi >= n_lo)) return fail(FFM_E_INVALID, "need 0 <= n_lo <= n_hi");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  if (int rc_e = eval_launch_pending(e)) return rc_e;
  hipLaunchKernelGGL(fill_state_kernel, dim3(2048), dim3(256), 0, e->stream, e->m, e->logical_len, seed, n_lo, n_hi, z_stddev);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  return FFM_OK;
}

int ffm_engine_eval_sigmoid(ffm_engine *e, int32_t n, const float *x, float *y) {
  if (!e || n < 0 || (n > 0 && (!x || !y))) return fail(FFM_E_INVALID, "bad argument");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  const int chunk = static_cast<int>(std::min<int64_t>(e->stage_floats / 2, 1 << 22));
  for (int off = 0; off < n; off += chunk) {
    const int c = std::min(chunk, n - off);
    HIP_TRY(hipMemcpyAsync(e->d_stage, x + off, sizeof(float) * c, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(sigmoid_eval_kernel, dim3(cdiv(c, 256)), dim3(256), 0, e->stream, c, e->d_stage, e->d_stage + chunk);
    HIP_TRY(hipMemcpyAsync(y + off, e->d_stage + chunk, sizeof(float) * c, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  return FFM_OK;
}

// Waits for the engine's stream, then reports (and clears) what the kernels flagged since the
// last report: the device entry points are asynchronous, so this is where their callers learn
// that a block could not be trained.
static int check_device_errors(ffm_engine *e) {
  int flags = 0;
  if (int rc_e = eval_launch_pending(e)) return rc_e;
  if (int rc_w = e->drain()) return rc_w;
  // the uploads of blocks that are staged but not trained yet run on the prep stream: the
  // zero-copy contract (include/ffm_engine.h) lets the caller reuse its page-locked arrays once
  // this returns, so they must have been pulled too
  for (int i = 0; i < e->n_staged; i++) HIP_TRY(hipEventSynchronize(e->slots[e->staged[i]].ev_copied));
  HIP_TRY(hipMemcpyAsync(&flags, e->d_err, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (flags) HIP_TRY(hipMemsetAsync(e->d_err, 0, sizeof(int), e->stream));
  if (flags & ERR_ROW_TOO_LONG)
    return fail(FFM_E_CAPACITY, "a row has more entries than max_row_nnz: its block was not trained "
                                "(outputs of that block are NaN)");
  if (flags & ERR_FIELD_MAP)
    return fail(FFM_E_INVALID, "an entry's feature id lies outside its field's id range (field_start): "
                               "its block was not trained");
  if (flags & ERR_SORT_BARRIER)
    return fail(FFM_E_DEVICE, "the grouping's one-launch sort could not get its workgroups on the device "
                              "together (grid barrier timed out): its block was not trained; FFM_OWN_SORT=0 "
                              "selects the library sort");
  if (flags) return fail(FFM_E_DEVICE, "device error flags " + std::to_string(flags));
  return FFM_OK;
}

int ffm_engine_sync(ffm_engine *e) {
  if (!e) return fail(FFM_E_INVALID, "null engine");
  HIP_TRY(hipSetDevice(e->cfg.device_id));
  return check_device_errors(e);
}

int ffm_engine_check_errors(ffm_engine *e) { return ffm_engine_sync(e); }

void *ffm_engine_stream(ffm_engine *e) { return e ? static_cast<void *>(e->stream) : nullptr; }

// Who owns what under field-pair sharding (host arithmetic only, no device needed).
int32_t ffm_engine_default_batch_ramp(float w_alpha) {
  if (!(w_alpha > 1e-3f)) return 32;
  const double r = 32.0 * std::pow(8.0, std::log10(static_cast<double>(w_alpha) / 1e-3));  // x 8 per decade
  return static_cast<int32_t>(std::min(r, 1048576.0) + 0.5);
}

int ffm_engine_shard_plan(int32_t n_fields, int32_t n_shards, int32_t field_map, int32_t *pair_owner,
                          int32_t *lin_owner, int32_t *bias_owner) {
  if (n_fields <= 0 || n_shards <= 0) return fail(FFM_E_INVALID, "n_fields and n_shards must be positive");
  const ShardPlan p = make_shard_plan(n_fields, n_shards, field_map != 0);
  // self-check: every unordered pair has exactly one owner, symmetrically
  for (int fa = 0; fa < n_fields; fa++)
    for (int fb = 0; fb < n_fields; fb++) {
      int owner = -1, count = 0;
      for (int r = 0; r < n_shards; r++)
        if (p.owns(r, fa, fb)) { owner = r; count++; }
      if (count != 1 || !p.owns(owner, fb, fa)) return fail(FFM_E_UNSUPPORTED, "no field-pair partition for this shape");
      if (pair_owner) pair_owner[static_cast<size_t>(fa) * n_fields + fb] = owner;
    }
  if (lin_owner) for (int f = 0; f < n_fields; f++) lin_owner[f] = p.lin_owner[f];
  if (bias_owner) *bias_owner = p.bias_owner;
  return FFM_OK;
}

#include "engine_state.h"
#include "engine_hash.h"
#include "engine_norm.h"
#include "engine_step.h"
#include "engine_stage.h"
#include "engine_refresh.h"
#include "engine_serve.h"
#include "engine_delta.h"
#include "engine_profile.h"
#include "engine_metrics.h"
#include "engine_keyed.h"
#include "engine_sketch.h"
#include "engine_idcount.h"
#include "engine_valhist.h"
#include "engine_text.h"
#include "engine_rows.h"
#include "engine_ablate.h"
#include "engine_mask.h"
}  // extern "C"

#include "engine_group.h"
