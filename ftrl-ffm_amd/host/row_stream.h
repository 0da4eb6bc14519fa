// row_stream.h -- --device_rows true: one text file as a stream of blocks that lie in HBM, in FILE ORDER -- the twin
// of CsrStream (csr_stream.h) for the passes that feed an engine.  The host does nothing per byte but copy it:
// TextChunkStream (text_stream.h) fills one of two page-locked slots with whole lines, the device parses the bytes
// (ffm_textparse), the host gets the chunk's row boundaries and nothing else of it (the page-locked mirror of
// row_ptr), places the cuts CsrStream::next would have placed (row_cut.h), and a row cutter (ffm_rowcut) moves the
// rows of every segment into the block being assembled, in HBM (include/ffm_engine.h "Resident rows").  Chunk t + 1
// is copied and parsed while chunk t is consumed.  A chunk the device will not parse -- a line outside its grammar, a
// single line longer than a slot -- goes through parse_csr_range on the host, whole, and into the same block at the
// same position: so a malformed line prints the same `wrong input: ...` and the run ends the same way.
#pragma once
#include <functional>
#include <future>
#include <string>
#include <vector>

#include "../../include/ffm_engine.h"
#include "csr_reader.h"
#include "row_cut.h"
#include "text_stream.h"

namespace ftrl {

class RowStream {
 public:
  static constexpr int kRing = 4;  // block buffers: three blocks are in flight in the engine, one is being assembled
  // max_rows / max_nnz: what one engine call takes (a block never exceeds either); pass: train | eval | predict, for
  // the line rewind() prints.  pulled: the engine's ffm_engine_blocks_pulled -- a block buffer is written again once
  // the block that lived there has been pulled.
  RowStream(const std::string &path, const std::string &file_type, int n_threads, int device, size_t max_rows, size_t max_nnz,
            const std::string &pass, std::function<long long()> pulled);
  ~RowStream();
  RowStream(const RowStream &) = delete;
  RowStream &operator=(const RowStream &) = delete;
  // The next `want` rows (fewer at the end of the file, or where the entry budget max_nnz ends the block early) as a
  // closed block in HBM; 0 at the end.  A single row with more entries than max_nnz is refused with CsrStream's
  // std::length_error.  Hand the block to the engine, then say so: handed_over (its staging number is in the block).
  size_t next(size_t want, ffm_rows_block *out);
  void handed_over(const ffm_rows_block &blk) { seq_[static_cast<size_t>(blk.index)] = blk.seq; }
  // Back to the first line (the next epoch); prints
  // `device rows: <pass> C chunks, B bytes, H parsed by the host (first at byte N), K blocks`.
  void rewind();

 private:
  struct Chunk {
    TextChunk text;
    bool started = false;   // its parse is on the device's queue
    bool ready = false;     // its row boundaries are on the host
    bool on_device = false;  // parsed by the device (else: `part`)
    const int32_t *mirror = nullptr;
    CsrPart part;
    std::vector<int32_t> row_ptr;  // prefix sums of part.nnz
    RowCutChunk cut;
  };
  bool fetch(Chunk &c);     // the next chunk of the file, its parse started; false at the end
  // ... in two halves: the read (pread into the chunk's slot) on a thread of its own, beside the blocks the caller
  // cuts and hands over; the parse started by the caller's thread once the bytes are there (wait: now)
  void begin_read(Chunk &c);
  void finish_read(bool wait);
  void start_parse(Chunk &c);
  void make_ready(Chunk &c);
  const RowCutChunk *chunk_at(size_t ordinal);
  void take(const RowSegment &seg);

  bool has_field_ = false;
  size_t max_rows_, max_nnz_;
  std::string pass_;
  std::function<long long()> pulled_;
  TextChunkStream text_;
  std::future<bool> read_;  // (behind text_: it is waited for before text_ goes)
  Chunk *reading_ = nullptr;
  ffm_textparse *parser_ = nullptr;
  ffm_rowcut *cutter_ = nullptr;
  Chunk chunk_[2];          // chunk_[ordinal & 1]
  size_t cur_ord_ = 0;      // the chunk being consumed
  bool begun_ = false, have_cur_ = false, have_next_ = false;
  RowCutCursor cursor_;
  int ring_pos_ = 0;
  bool held_[kRing] = {false, false, false, false};
  long long seq_[kRing] = {0, 0, 0, 0};
  unsigned long long chunks_ = 0, bytes_ = 0, by_host_ = 0, first_host_ = 0, blocks_ = 0;
};

}  // namespace ftrl
