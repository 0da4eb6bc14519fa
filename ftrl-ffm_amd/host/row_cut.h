// row_cut.h -- --device_rows true: where the blocks of a file end, from the chunks' row boundaries alone.  Pure host
// code (no HIP, no engine): the cut rule of CsrStream::next (csr_stream.cpp) over chunks of which the host holds
// nothing but row_ptr -- the page-locked mirror of a chunk the device parsed (include/ffm_engine.h "Resident rows"),
// or the prefix sums of one the host parsed.  A block is `want` rows at the most and `max_nnz` entries at the most; it
// ends early rather than exceed the entry budget; a single row over the budget goes out alone, or is refused with
// CsrStream's std::length_error where the block cannot grow (fixed_capacity).
//
// The planner asks for chunks by their ordinal and hands out every segment -- rows [r0, r1) of one chunk -- the
// moment it is decided, in file order: the device holds two chunks at a time, so the rows of chunk t are taken before
// chunk t + 2 is asked for (the caller may then parse into chunk t's slot).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <stdexcept>

namespace ftrl {

// A chunk as the planner sees it: row_ptr [n_rows + 1], non-decreasing (it may start at any value).
struct RowCutChunk {
  const int32_t *row_ptr = nullptr;
  size_t n_rows = 0;
};

struct RowSegment {
  size_t chunk = 0;     // the chunk's ordinal
  size_t r0 = 0, r1 = 0;  // its rows [r0, r1)
  size_t nnz = 0;       // their entries
};

// Where the next block begins.
struct RowCutCursor {
  size_t chunk = 0, row = 0;
};

// Plans one block from `cur` on.  chunk_at(ordinal) -> const RowCutChunk * (nullptr: the file has no such chunk);
// asked for ordinals in order, for ordinal t + 1 only after every segment of chunk t was emitted.  emit(segment) is
// called once per segment.  Returns the block's rows (0: the end of the file); *nnz_out: its entries.
template <class ChunkAt, class Emit>
size_t plan_block(size_t want, size_t max_nnz, bool fixed_capacity, RowCutCursor &cur, ChunkAt &&chunk_at, Emit &&emit,
                  size_t *nnz_out = nullptr) {
  size_t got = 0, nnz = 0;
  while (got < want) {
    const RowCutChunk *c = chunk_at(cur.chunk);
    if (!c) break;
    if (cur.row >= c->n_rows) {  // (a chunk of blank lines)
      cur.chunk++;
      cur.row = 0;
      continue;
    }
    const int32_t *rp = c->row_ptr + cur.row;
    auto entries = [&](size_t t) { return static_cast<size_t>(rp[t] - rp[0]); };
    size_t take = std::min(want - got, c->n_rows - cur.row);
    bool cut = false;  // the entry budget ends the block here
    while (take > 0 && nnz + entries(take) > max_nnz) { take--; cut = true; }
    if (take == 0) {
      if (got > 0) break;
      if (fixed_capacity) throw std::length_error("a row has more entries than a block can hold (max_nnz)");
      take = 1;  // (a growable block: the row goes out alone)
    }
    RowSegment seg;
    seg.chunk = cur.chunk;
    seg.r0 = cur.row;
    seg.r1 = cur.row + take;
    seg.nnz = entries(take);
    emit(seg);
    nnz += seg.nnz;
    got += take;
    cur.row += take;
    if (cur.row == c->n_rows) {
      cur.chunk++;
      cur.row = 0;
    }
    if (cut) break;
  }
  if (nnz_out) *nnz_out = nnz;
  return got;
}

}  // namespace ftrl
