// kernels_stage.h -- rows streaming between host memory and the staging slots inside the training loop: the
// upload kernel (one template: plain, weighted, hashed, without values) and the score download kernel.
// Their launches and the slots' bookkeeping are host code: engine_stage.h.
#pragma once
#include <tuple>
#include <type_traits>

#include "hash_ids.h"

namespace ftrl_dev {

// Upload of one staged block by a kernel: the five CSR arrays are read straight out of page-locked
// (device-mapped) host memory, 16 bytes per lane, and written to the staging slot's device arrays.
// A hipMemcpyAsync here makes the SUBMITTING THREAD wait until the stream's earlier kernels have
// finished (measured: mean 0.38 ms, up to 16 ms per call) -- the host then cannot run ahead of the
// GPU and every other step starts ~230 us late; a kernel launch never blocks.
// Every wave starts with a system-scope acquire (it drops the non-coherent lines of its L2): a
// caller that refills a block buffer it has used before (the trainers' ring) must not be served
// lines of the previous block that are still on-die, should the runtime map its page-locked memory
// cacheable.  (System-scope LOADS instead -- 8 bytes per lane -- halved the upload rate.)
struct PullJob {
  const char *src[5]; char *dst[5]; unsigned bytes[5];
  long long ordinal; long long *pulled; unsigned *ticket;  // completion word (host memory), see h_pulled
  // rows handed over without a field array (one entry per field in field order): the slot's field
  // array is written here -- entry j of the block is field j mod n_fields -- instead of crossing PCIe
  int *gen_field; unsigned gen_n; int gen_fields;
};
// A block with sample weights: the sixth array, n_rows floats, moves with the other five (whole 16-byte
// vectors, then the last n_rows % 4 floats as single words).
struct PullWeightedJob { PullJob block; const char *wsrc; char *wdst; unsigned wbytes; };
// FFM_FLAG_HASH_IDS: the ids are hashed on their way through (csrc/hash_ids.h).  feat and field are taken
// out of the block's five arrays (their byte counts there are 0) and move in ONE loop instead: they are
// equally long, so a lane loads the int4 of feat and the int4 of field, hashes four entries and stores
// both; the last nnz % 4 entries go one by one.  No byte crosses PCIe twice, and the integer work hides
// behind the link (the kernel is bound by PCIe).  fsrc == nullptr: no field array came -- LR / FM, or FFM
// rows of one entry per field in field order, whose fields the kernel's end writes (gen_field) and this
// loop recomputes the same way.
struct PullHashJob {
  PullWeightedJob w;
  ftrl_hash::Map hm;
  const char *isrc, *fsrc; char *idst, *fdst; unsigned hbytes;
};
// A flagged engine with a keep-map (include/ffm_engine.h "Rare ids"): the hashed loop folds every entry by the
// map before it hashes it (ftrl_hash::hash_entry_rare).  The map and its shift stand behind the hashed job, so
// an engine without a map hands over the PullHashJob it always did.
struct PullRareJob { PullHashJob h; ftrl_hash::Rare rare; };
// A flagged FFM engine with a bucket table (include/ffm_engine.h "Value buckets"): val too is taken out of the
// block's five arrays and moves in the hashed loop, which maps (field, id, value) to (field, id', value')
// (ftrl_hash::hash_entry_bucket).  vsrc == nullptr: the block brought no values, every one is 1.0f -- the loop
// writes the slot's val array itself, so these instantiations take no Ones.  rare.words == nullptr: no keep-map
// (a run-time branch here, where the bucketing work is anyway).
struct PullBucketPart { ftrl_hash::Buckets bk; const char *vsrc; char *vdst; };
struct PullBucketJob { PullRareJob r; PullBucketPart b; };

// What an instantiation takes: the smallest of the three jobs that holds its parts.  Every variant is a
// kernel of its own -- an instantiation, not a run-time branch -- so that a block without weights, on an
// unflagged engine, with its values is uploaded by the launch, the argument and the kernel it always was
// (profiles/sample_weights.md, profiles/implicit_ones.md).
template <bool WEIGHTED, bool HASHED, bool RARE, bool BUCKET>
using PullArg = std::conditional_t<BUCKET, PullBucketJob, std::conditional_t<RARE, PullRareJob, std::conditional_t<HASHED, PullHashJob, std::conditional_t<WEIGHTED, PullWeightedJob, PullJob>>>>;

// Ones: nothing, or <float *, unsigned> = the slot's val array and the number of 1.0f to write there.
// The parts in order: the five arrays, the weights, the hashed loop, the ones, a missing field array, the ticket.
// The copy of an array is spelled out where it is used, for the five and for the weights: as a
// `__device__ __forceinline__` function the same text is scheduled differently (every variant keeps its
// registers but not its instruction count), and so is the job when a function hands out its inner parts by
// reference -- hence the two pointers picked by `if constexpr`.  As it stands every instantiation compiles to
// the instructions of the kernel it replaces.
// RARE (with HASHED only): the hashed loop below runs on the job's hashed part and folds by the job's map.
// BUCKET (with HASHED, without RARE and without Ones): the hashed loop's third text, at the end of the three.
template <bool WEIGHTED, bool HASHED, bool RARE, bool BUCKET, typename... Ones>
__global__ __launch_bounds__(256) void pull_block_kernel(PullArg<WEIGHTED, HASHED, RARE, BUCKET> arg, Ones... ones) {
  static_assert(sizeof...(Ones) == 0 || sizeof...(Ones) == 2, "Ones: nothing, or <float *, unsigned>");
  static_assert(HASHED || !RARE, "RARE: a variant of the hashed loop");
  static_assert(!BUCKET || (HASHED && !RARE && sizeof...(Ones) == 0), "BUCKET: a variant of the hashed loop that holds the fold and the ones");
  const PullJob *block;
  if constexpr (BUCKET) block = &arg.r.h.w.block; else if constexpr (RARE) block = &arg.h.w.block; else if constexpr (HASHED) block = &arg.w.block; else if constexpr (WEIGHTED) block = &arg.block; else block = &arg;
  const PullJob &job = *block;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
  const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
#pragma unroll
  for (int a = 0; a < 5; a++) {
    const unsigned n16 = job.bytes[a] >> 4;
    const int4 *s = reinterpret_cast<const int4 *>(job.src[a]);
    int4 *d = reinterpret_cast<int4 *>(job.dst[a]);
    // (one load per lane in flight: two, four and eight measured the same -- 42 GB/s is what a kernel reads over PCIe here)
    for (unsigned i = tid; i < n16; i += stride) d[i] = s[i];
    const unsigned tail = job.bytes[a] & 15u;  // sizes are multiples of 4
    if (tid < (tail >> 2))
      reinterpret_cast<int *>(job.dst[a])[(n16 << 2) + tid] = reinterpret_cast<const int *>(job.src[a])[(n16 << 2) + tid];
  }
  if constexpr (WEIGHTED) {
    const PullWeightedJob *weights;
    if constexpr (BUCKET) weights = &arg.r.h.w; else if constexpr (RARE) weights = &arg.h.w; else if constexpr (HASHED) weights = &arg.w; else weights = &arg;
    const PullWeightedJob &wj = *weights;
    const unsigned n16 = wj.wbytes >> 4;
    const int4 *s = reinterpret_cast<const int4 *>(wj.wsrc);
    int4 *d = reinterpret_cast<int4 *>(wj.wdst);
    for (unsigned i = tid; i < n16; i += stride) d[i] = s[i];
    const unsigned tail = wj.wbytes & 15u;
    if (tid < (tail >> 2))
      reinterpret_cast<int *>(wj.wdst)[(n16 << 2) + tid] = reinterpret_cast<const int *>(wj.wsrc)[(n16 << 2) + tid];
  }
  if constexpr (HASHED && !RARE && !BUCKET) {
    const unsigned n16 = arg.hbytes >> 4, F = static_cast<unsigned>(arg.hm.n_fields);
    for (unsigned i = tid; i < n16; i += stride) {
      const int4 ft = reinterpret_cast<const int4 *>(arg.isrc)[i];
      int4 fl;
      if (arg.fsrc) {
        fl = reinterpret_cast<const int4 *>(arg.fsrc)[i];
        reinterpret_cast<int4 *>(arg.fdst)[i] = fl;
      } else fl = arg.hm.ffm ? ftrl_hash::hash_implicit_fields4(i, F) : make_int4(0, 0, 0, 0);
      reinterpret_cast<int4 *>(arg.idst)[i] = ftrl_hash::hash_entries4(arg.hm, fl, ft);
    }
    if (tid < ((arg.hbytes & 15u) >> 2)) {
      const unsigned p = (n16 << 2) + tid;
      int f = arg.hm.ffm ? static_cast<int>(p % F) : 0;
      if (arg.fsrc) {
        f = reinterpret_cast<const int *>(arg.fsrc)[p];
        reinterpret_cast<int *>(arg.fdst)[p] = f;
      }
      reinterpret_cast<int *>(arg.idst)[p] = ftrl_hash::hash_entry(arg.hm, f, reinterpret_cast<const int *>(arg.isrc)[p]);
    }
  }
  // (the hashed loop once more, folding.  Its own text: as ONE loop that picks the job's hashed part and the entry
  // function by `if constexpr`, the two unweighted hashed instantiations above came out two instructions longer than
  // the kernels they replace -- the effect the comment ahead of the kernel describes)
  if constexpr (RARE) {
    const PullHashJob &hj = arg.h;
    const unsigned n16 = hj.hbytes >> 4, F = static_cast<unsigned>(hj.hm.n_fields);
    for (unsigned i = tid; i < n16; i += stride) {
      const int4 ft = reinterpret_cast<const int4 *>(hj.isrc)[i];
      int4 fl;
      if (hj.fsrc) {
        fl = reinterpret_cast<const int4 *>(hj.fsrc)[i];
        reinterpret_cast<int4 *>(hj.fdst)[i] = fl;
      } else fl = hj.hm.ffm ? ftrl_hash::hash_implicit_fields4(i, F) : make_int4(0, 0, 0, 0);
      reinterpret_cast<int4 *>(hj.idst)[i] = ftrl_hash::hash_entries4_rare(hj.hm, arg.rare, fl, ft);
    }
    if (tid < ((hj.hbytes & 15u) >> 2)) {
      const unsigned p = (n16 << 2) + tid;
      int f = hj.hm.ffm ? static_cast<int>(p % F) : 0;
      if (hj.fsrc) {
        f = reinterpret_cast<const int *>(hj.fsrc)[p];
        reinterpret_cast<int *>(hj.fdst)[p] = f;
      }
      reinterpret_cast<int *>(hj.idst)[p] = ftrl_hash::hash_entry_rare(hj.hm, arg.rare, f, reinterpret_cast<const int *>(hj.isrc)[p]);
    }
  }
  // (and once more, bucketing: val moves here too -- loaded, or 1.0f where the block brought none -- and every
  // entry stores its field, its model id and its value)
  if constexpr (BUCKET) {
    const PullHashJob &hj = arg.r.h;
    const PullBucketPart &bp = arg.b;
    const unsigned n16 = hj.hbytes >> 4, F = static_cast<unsigned>(hj.hm.n_fields);
    for (unsigned i = tid; i < n16; i += stride) {
      const int4 ft = reinterpret_cast<const int4 *>(hj.isrc)[i];
      int4 fl;
      if (hj.fsrc) {
        fl = reinterpret_cast<const int4 *>(hj.fsrc)[i];
        reinterpret_cast<int4 *>(hj.fdst)[i] = fl;
      } else fl = ftrl_hash::hash_implicit_fields4(i, F);
      uint4 v = make_uint4(ftrl_hash::kOneBits, ftrl_hash::kOneBits, ftrl_hash::kOneBits, ftrl_hash::kOneBits);
      if (bp.vsrc) v = reinterpret_cast<const uint4 *>(bp.vsrc)[i];
      reinterpret_cast<int4 *>(hj.idst)[i] = ftrl_hash::hash_entries4_bucket(hj.hm, arg.r.rare, bp.bk, fl, ft, &v);
      reinterpret_cast<uint4 *>(bp.vdst)[i] = v;
    }
    if (tid < ((hj.hbytes & 15u) >> 2)) {
      const unsigned p = (n16 << 2) + tid;
      int f = static_cast<int>(p % F);
      if (hj.fsrc) {
        f = reinterpret_cast<const int *>(hj.fsrc)[p];
        reinterpret_cast<int *>(hj.fdst)[p] = f;
      }
      unsigned v = bp.vsrc ? reinterpret_cast<const unsigned *>(bp.vsrc)[p] : ftrl_hash::kOneBits;
      reinterpret_cast<int *>(hj.idst)[p] = ftrl_hash::hash_entry_bucket(hj.hm, arg.r.rare, bp.bk, f, reinterpret_cast<const int *>(hj.isrc)[p], &v);
      reinterpret_cast<unsigned *>(bp.vdst)[p] = v;
    }
  }
  // A block handed over without values (val == NULL: every value is 1.0f, include/ffm_engine.h "Rows without
  // values"): nothing of val is in the job's five arrays, and the upload writes the slot's val array itself,
  // over its own grid stride, the way it writes a missing field array below -- a lane stores four 1.0f as one
  // 16-byte vector, the last n % 4 go singly.  The stores hide behind the link (the kernel is bound by PCIe).
  // Every such block writes them again: a block that brought its values may have used the slot in between.
  if constexpr (sizeof...(Ones) != 0) {
    const auto [dst, n] = std::tuple<Ones...>(ones...);
    const unsigned n4 = n >> 2;
    const float4 ones4 = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    for (unsigned i = tid; i < n4; i += stride) reinterpret_cast<float4 *>(dst)[i] = ones4;
    if (tid < (n & 3u)) dst[(n4 << 2) + tid] = 1.0f;
  }
  if (job.gen_n) {
    const unsigned n4 = job.gen_n >> 2, F = static_cast<unsigned>(job.gen_fields);
    for (unsigned i = tid; i < n4; i += stride) reinterpret_cast<int4 *>(job.gen_field)[i] = ftrl_hash::hash_implicit_fields4(i, F);
    if (tid < (job.gen_n & 3u)) job.gen_field[(n4 << 2) + tid] = static_cast<int>(((n4 << 2) + tid) % F);
  }
  // the workgroup that finishes last publishes the block's number to the host
  __syncthreads();  // (every load of this workgroup has returned: its stores were issued after them)
  if (threadIdx.x == 0) {
    __threadfence();
    if (atomicAdd(job.ticket, 1u) == gridDim.x - 1) {
      *job.ticket = 0u;
      __hip_atomic_store(job.pulled, job.ordinal, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// The mirror image of the upload: the scores of one predicted block go from e->d_out to the caller's
// page-locked (device-mapped) host memory, 16 bytes per lane -- a lane carries four rows --, the last
// n % 4 floats as single stores.  A kernel for the reason pull_block_kernel is one: a hipMemcpyAsync
// makes the submitting thread wait for the stream's earlier kernels.  Launched on the MAIN stream
// right behind the block's predict kernel (eval_launch_pending), so it needs no event.
// The stores leave the device: every lane follows its own with a system-scope release fence (the
// upload's agent-scope __threadfence() orders nothing towards the host), and the workgroup that
// finishes last publishes the block's staging number into h_scored, again at system scope -- a host
// that reads the number (ffm_engine_blocks_scored, an acquire load) then reads whole scores.
// It writes n floats and nothing behind them.
struct PushJob {
  const float *src; float *dst; unsigned n;
  long long ordinal; long long *scored; unsigned *ticket;  // completion word (host memory), see h_scored
};
__global__ __launch_bounds__(256) void push_scores_kernel(PushJob job) {
  const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  const unsigned n4 = job.n >> 2;
  const float4 *s = reinterpret_cast<const float4 *>(job.src);
  float4 *d = reinterpret_cast<float4 *>(job.dst);
  for (unsigned i = tid; i < n4; i += stride) d[i] = s[i];
  if (tid < (job.n & 3u)) job.dst[(n4 << 2) + tid] = job.src[(n4 << 2) + tid];
  __threadfence_system();
  __syncthreads();  // (every wave of this workgroup is past its fence: its scores are in host memory)
  if (threadIdx.x == 0) {
    if (__hip_atomic_fetch_add(job.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
      *job.ticket = 0u;
      __hip_atomic_store(job.scored, job.ordinal, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

}  // namespace ftrl_dev
