// count_block.h -- the block a counting pre-pass over the training file fills (field_count.cpp, rare_count.cpp,
// value_count.cpp): its field and feat arrays -- and val, where the pass reads values -- page-locked at their capacity,
// so that the device reads the entries where the parser's threads wrote them; the other arrays stay pageable.
#pragma once
#include "../../include/ffm_engine.h"
#include "csr_stream.h"

namespace ftrl {

// rows / entries of one counted block: large, so that the launch and the wait per block stay small beside its parse
constexpr size_t kCountRows = 32768, kCountNnz = kCountRows * 64;

struct CountBlock {
  CsrBlock blk;
  bool pinned = false;  // (false: no page-locked memory to be had -- the counting object copies each block into its own)
  bool pinned_val = false;
  explicit CountBlock(bool with_val = false) {
    blk.row_ptr.reserve(kCountRows + 1);
    blk.label.reserve(kCountRows);
    blk.field.reserve(kCountNnz);
    blk.feat.reserve(kCountNnz);
    blk.val.reserve(kCountNnz);
    auto pages = [](size_t n) { return (4 * n + 4095) & ~static_cast<size_t>(4095); };  // (PageAllocator's)
    if (ffm_engine_pin_host(blk.field.data(), pages(blk.field.capacity())) != FFM_OK) return;
    if (ffm_engine_pin_host(blk.feat.data(), pages(blk.feat.capacity())) != FFM_OK) {
      ffm_engine_unpin_host(blk.field.data());
      return;
    }
    if (with_val) {
      if (ffm_engine_pin_host(blk.val.data(), pages(blk.val.capacity())) != FFM_OK) {
        ffm_engine_unpin_host(blk.field.data());
        ffm_engine_unpin_host(blk.feat.data());
        return;
      }
      pinned_val = true;
    }
    pinned = true;
  }
  ~CountBlock() {
    if (!pinned) return;
    ffm_engine_unpin_host(blk.field.data());
    ffm_engine_unpin_host(blk.feat.data());
    if (pinned_val) ffm_engine_unpin_host(blk.val.data());
  }
  CountBlock(const CountBlock &) = delete;
  CountBlock &operator=(const CountBlock &) = delete;
};

}  // namespace ftrl
