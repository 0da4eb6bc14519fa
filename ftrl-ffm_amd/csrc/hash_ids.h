// hash_ids.h -- the hashing trick, per field: id' = lo[f] + h(f, id) mod-like-into width[f], IDENTICAL
// BITS on the device and on the host (the contract is stated in include/ffm_engine.h, "Hashed ids").
//
// The reference has no counterpart: FtrlModel::remove_out_range / FFM::remove_out_range
// (ftrl_model.cpp:36-42, ffm.cpp:30-36) erase every id >= n_feats, so a file whose id space is larger than
// the model trains on a fraction of its entries.  Here such an id is folded into the range of its field
// instead -- which also gives any data the one-range-per-field layout the compact shards, the range sort
// and the regular-block forms are built around.  Unsigned 32-bit wrap-around arithmetic only, then one
// 32 x 32 -> 64 multiply whose high half scales the hash into [0, width): no divide, no table.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FTRL_HASH_HD __host__ __device__ __forceinline__
#else
#define FTRL_HASH_HD inline
#endif

namespace ftrl_hash {

FTRL_HASH_HD uint32_t mix32(uint32_t x) {  // the murmur3 finaliser
  x ^= x >> 16;
  x *= 0x85ebca6bu;
  x ^= x >> 13;
  x *= 0xc2b2ae35u;
  x ^= x >> 16;
  return x;
}

// The 32 hashed bits of a valid entry: `field` salts the hash (0 for LR / FM).  mix32 is a bijection, so two
// ids of one field never share them (what the field sketches count, kernels_sketch.h).
FTRL_HASH_HD uint32_t hash_bits(int32_t field, int32_t feat) {
  const uint32_t salt = (static_cast<uint32_t>(field) + 1u) * 0x9e3779b9u;  // ((uint32)(field + 1), without signed overflow)
  return mix32(static_cast<uint32_t>(feat) ^ salt);
}

// A valid entry's model id: [lo, lo + width) is where its hashed bits land.
FTRL_HASH_HD int32_t hash_into(int32_t field, int32_t feat, int32_t lo, uint32_t width) {
  const uint32_t x = hash_bits(field, feat);
  return lo + static_cast<int32_t>((static_cast<uint64_t>(x) * static_cast<uint64_t>(width)) >> 32);
}

// Where the ids of a model go: `start` = the fields' id ranges (n_fields + 1 ascending values; FFM with
// field_start) or null = one range [0, n_feats); ffm: fields are checked and salt the hash.
struct Map {
  const int32_t *start;
  int32_t n_feats, n_fields, ffm;
};

// One entry.  Entries the reference erases stay erased: a negative id, or (FFM) a field outside
// [0, n_fields), gives -1, which every kernel downstream drops as it drops any id outside [0, n_feats).
FTRL_HASH_HD int32_t hash_entry(const Map &m, int32_t field, int32_t feat) {
  if (feat < 0) return -1;
  if (!m.ffm) return hash_into(0, feat, 0, static_cast<uint32_t>(m.n_feats));
  if (static_cast<uint32_t>(field) >= static_cast<uint32_t>(m.n_fields)) return -1;
  if (!m.start) return hash_into(field, feat, 0, static_cast<uint32_t>(m.n_feats));
  const int32_t lo = m.start[field];
  return hash_into(field, feat, lo, static_cast<uint32_t>(m.start[field + 1] - lo));
}

// Rare ids (include/ffm_engine.h "Rare ids"): a keep-map of 2^bits slots, bit j of word i = slot 64 i + j, and
// shift = 32 - bits.  An entry's slot is the top `bits` of its hashed bits.  Beside Map, never inside it: the
// kernels of an engine without a map take the Map they always took.
constexpr int32_t kRareId = 0x7fffffff;  // FFM_RARE_ID
struct Rare {
  const uint64_t *words;
  uint32_t shift;
};
FTRL_HASH_HD bool rare_kept(const Rare &r, int32_t field, int32_t feat) {
  const uint32_t slot = hash_bits(field, feat) >> r.shift;
  return (r.words[slot >> 6] >> (slot & 63u)) & 1u;
}
// The raw id the hash then takes: kRareId for a counting entry (feat >= 0 and, for FFM, 0 <= field < n_fields;
// LR / FM: field taken as 0) whose slot's bit is 0, feat for every other entry.
FTRL_HASH_HD int32_t fold_entry(bool ffm, int32_t n_fields, const Rare &r, int32_t field, int32_t feat) {
  if (feat < 0) return feat;
  if (!ffm) field = 0;
  else if (static_cast<uint32_t>(field) >= static_cast<uint32_t>(n_fields)) return feat;
  return rare_kept(r, field, feat) ? feat : kRareId;
}
FTRL_HASH_HD int32_t hash_entry_rare(const Map &m, const Rare &r, int32_t field, int32_t feat) {
  return hash_entry(m, field, fold_entry(m.ffm != 0, m.n_fields, r, field, feat));
}

// Value buckets (include/ffm_engine.h "Value buckets"): a numeric column's value, taken by its bit pattern, gives
// one of 65536 order-preserving bins; a field's table of at most 255 ascending bins (its edges) cuts them into
// buckets, and a bucketed entry becomes (bucket, 1.0f).  Integer instructions only.  Beside Map and Rare, never
// inside them: the kernels of an engine without a table take what they always took.
constexpr int32_t kBucketBins = 65536, kBucketMaxEdges = 255, kBucketNanId = 65536;  // FFM_BUCKET_*
constexpr uint32_t kOneBits = 0x3f800000u;  // 1.0f
FTRL_HASH_HD bool value_is_nan(uint32_t u) { return (u & 0x7fffffffu) > 0x7f800000u; }
FTRL_HASH_HD uint32_t value_bin(uint32_t u) {
  if ((u & 0x7fffffffu) == 0u) u = 0u;  // (-0.0 and +0.0: one key)
  return ((u >> 31) ? ~u : (u | 0x80000000u)) >> 16;
}
// n_edges[f]: -1 = field f is not bucketed, else its number of edges; edges[f * kBucketMaxEdges ..]: its edges.
struct Buckets {
  const int32_t *n_edges;
  const uint16_t *edges;
};
// The number of edges < bin: a binary search of at most 8 steps (n <= 255).
FTRL_HASH_HD int32_t bucket_of(const uint16_t *edges, int32_t n, uint32_t bin) {
  int32_t lo = 0, hi = n;
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    if (edges[mid] < bin) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// One entry: true iff it is bucketed (feat >= 0, 0 <= field < n_fields, the field has a table); *feat and *vbits
// (the value's bits) are then replaced.  Every other entry is left as it is.
FTRL_HASH_HD bool bucket_entry(int32_t n_fields, const Buckets &b, int32_t field, int32_t *feat, uint32_t *vbits) {
  if (*feat < 0 || static_cast<uint32_t>(field) >= static_cast<uint32_t>(n_fields)) return false;
  const int32_t n = b.n_edges[field];
  if (n < 0) return false;
  *feat = value_is_nan(*vbits) ? kBucketNanId : bucket_of(b.edges + field * kBucketMaxEdges, n, value_bin(*vbits));
  *vbits = kOneBits;
  return true;
}
// An engine's whole mapping of one FFM entry: bucket, else fold (r.words != nullptr), then hash.  Returns the model
// id; *vbits is the value the kernels downstream take.
FTRL_HASH_HD int32_t hash_entry_bucket(const Map &m, const Rare &r, const Buckets &b, int32_t field, int32_t feat, uint32_t *vbits) {
  if (bucket_entry(m.n_fields, b, field, &feat, vbits)) return hash_entry(m, field, feat);
  return r.words ? hash_entry_rare(m, r, field, feat) : hash_entry(m, field, feat);
}

#if defined(__HIPCC__)
// Four entries at a time, for the kernels that carry them as 16-byte vectors (hash_ids_kernel, the upload kernel).
// The fields of entries 4i .. 4i + 3 of a block handed over without a field array: one entry per field in
// field order, so entry p is field p mod n_fields (what the upload kernel writes as the slot's field array).
__device__ __forceinline__ int4 hash_implicit_fields4(unsigned i, unsigned F) {
  const unsigned f0 = (4u * i) % F, f1 = f0 + 1u < F ? f0 + 1u : 0u, f2 = f1 + 1u < F ? f1 + 1u : 0u;
  return make_int4(static_cast<int>(f0), static_cast<int>(f1), static_cast<int>(f2), static_cast<int>(f2 + 1u < F ? f2 + 1u : 0u));
}
__device__ __forceinline__ int4 hash_entries4(const Map &hm, const int4 fl, const int4 ft) {
  return make_int4(hash_entry(hm, fl.x, ft.x), hash_entry(hm, fl.y, ft.y), hash_entry(hm, fl.z, ft.z), hash_entry(hm, fl.w, ft.w));
}
__device__ __forceinline__ int4 hash_entries4_rare(const Map &hm, const Rare &r, const int4 fl, const int4 ft) {
  return make_int4(hash_entry_rare(hm, r, fl.x, ft.x), hash_entry_rare(hm, r, fl.y, ft.y), hash_entry_rare(hm, r, fl.z, ft.z),
                   hash_entry_rare(hm, r, fl.w, ft.w));
}
// ... bucketing: v = the four values' bits, replaced where an entry is bucketed.
__device__ __forceinline__ int4 hash_entries4_bucket(const Map &hm, const Rare &r, const Buckets &b, const int4 fl, const int4 ft, uint4 *v) {
  return make_int4(hash_entry_bucket(hm, r, b, fl.x, ft.x, &v->x), hash_entry_bucket(hm, r, b, fl.y, ft.y, &v->y),
                   hash_entry_bucket(hm, r, b, fl.z, ft.z, &v->z), hash_entry_bucket(hm, r, b, fl.w, ft.w, &v->w));
}
#endif

}  // namespace ftrl_hash
