// types.h -- row types of the host interface; same shapes as the reference's
// src/include/utils/types.h:18-25 and src/include/data/sample.h:6-9 so callers port unchanged.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <new>
#include <tuple>
#include <vector>

typedef int8_t int8;
typedef int16_t int16;
typedef int32_t int32;
typedef int64_t int64;
typedef uint8_t uint8;
typedef uint16_t uint16;
typedef uint32_t uint32;
typedef uint64_t uint64;

typedef std::tuple<int, int, float> feat;  // (field, feat, value)
typedef std::vector<feat> feat_vec;

enum class ModelType : uint8_t { LR = 0, FM = 1, FFM = 2 };

struct Sample {
  feat_vec x;
  int y;
};

// Whole pages per array: a block's arrays can then be page-locked one by one (hipHostRegister
// works on pages: two small arrays sharing a heap page cannot both be registered).
template <typename T>
struct PageAllocator {
  using value_type = T;
  PageAllocator() = default;
  template <typename U> PageAllocator(const PageAllocator<U> &) {}
  T *allocate(size_t n) {
    const size_t bytes = (n * sizeof(T) + 4095) & ~static_cast<size_t>(4095);
    void *p = std::aligned_alloc(4096, bytes ? bytes : 4096);
    if (!p) throw std::bad_alloc();
    return static_cast<T *>(p);
  }
  void deallocate(T *p, size_t) { std::free(p); }
  template <typename U> bool operator==(const PageAllocator<U> &) const { return true; }
  template <typename U> bool operator!=(const PageAllocator<U> &) const { return false; }
};

// What the readers note about a row while they write its entries (one byte per row; a block's two facts are
// the AND over its rows): every value's bits are 1.0f; the entries' fields are 0, 1, ..., len - 1 in that order.
constexpr uint8_t kRowOnes = 1, kRowOrdered = 2;
inline bool is_one_bits(float v) {
  uint32_t b;
  __builtin_memcpy(&b, &v, sizeof b);
  return b == 0x3f800000u;
}

// A block of rows in the engine's CSR wire format (include/ffm_engine.h).
struct CsrBlock {
  std::vector<int32_t, PageAllocator<int32_t>> row_ptr{0}, field, feat, label;
  std::vector<float, PageAllocator<float>> val;
  // sample weights, one per row (include/ffm_engine.h "Sample weights"), or empty: an unweighted block
  std::vector<float, PageAllocator<float>> weight;
  // Two facts about the block, kept up to date by whoever writes its entries (note_row; no second pass):
  // every value's bits are 1.0f -- the block may cross PCIe without its val array -- and, with all_ordered,
  // every row has row_len entries whose fields are 0 .. row_len - 1 in order: with row_len == n_fields an FFM
  // block may go without its field array (include/ffm_engine.h: val == NULL, field == NULL).
  // A block that nobody cleared claims neither (its arrays may have been written directly); clear() starts both.
  bool all_ones = false, all_ordered = false;
  int32_t row_len = -1;  // the rows' common length; -1: no row yet, -2: the rows differ
  int32_t n_rows() const { return static_cast<int32_t>(row_ptr.size()) - 1; }
  bool one_entry_per_field(int n_fields) const { return all_ordered && (row_len == n_fields || row_len == -1); }
  void reset_facts() { all_ones = all_ordered = true; row_len = -1; }
  void forget_facts() { all_ones = all_ordered = false; }  // (its arrays were written by someone who kept no track)
  // a run of `whole`'s rows (a block split for capacity): what holds of every row holds of these
  void inherit_facts(const CsrBlock &whole) { all_ones = whole.all_ones; all_ordered = whole.all_ordered; row_len = whole.row_len; }
  void note_row(uint8_t row_flags, int32_t len) {
    all_ones = all_ones && (row_flags & kRowOnes);
    all_ordered = all_ordered && (row_flags & kRowOrdered);
    row_len = row_len == -1 || row_len == len ? len : -2;
  }
  void clear() {
    row_ptr.assign(1, 0);
    field.clear(); feat.clear(); label.clear(); val.clear(); weight.clear();
    reset_facts();
  }
  void push(const Sample &s) {
    uint8_t flags = kRowOnes | kRowOrdered;
    int32_t n = 0;
    for (const auto &[f, i, v] : s.x) {
      if (!is_one_bits(v)) flags &= static_cast<uint8_t>(~kRowOnes);
      if (f != n++) flags &= static_cast<uint8_t>(~kRowOrdered);
      field.push_back(f); feat.push_back(i); val.push_back(v);
    }
    note_row(flags, n);
    row_ptr.push_back(static_cast<int32_t>(feat.size()));
    label.push_back(s.y);
  }
};
