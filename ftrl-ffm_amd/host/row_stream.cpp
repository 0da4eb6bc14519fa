#include "row_stream.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <stdexcept>
#include <thread>

namespace ftrl {

namespace {

void check_rc(int rc, const char *what) {
  if (rc != FFM_OK) throw std::runtime_error(std::string(what) + ": " + ffm_engine_last_error());
}

}  // namespace

RowStream::RowStream(const std::string &path, const std::string &file_type, int n_threads, int device, size_t max_rows, size_t max_nnz,
                     const std::string &pass, std::function<long long()> pulled)
    : has_field_(file_type == "libffm"), max_rows_(max_rows), max_nnz_(max_nnz), pass_(pass), pulled_(std::move(pulled)),
      text_(path, n_threads, TextChunkStream::slot_bytes_from_env()) {
  // capacities no chunk can exceed: a row is at least 2 bytes of text ("1\n"), an entry at least 4 ("1:1 ")
  const size_t B = text_.slot_bytes();
  check_rc(ffm_engine_textparse_create(has_field_ ? 1 : 0, static_cast<int64_t>(B), static_cast<int32_t>(B / 2 + 1), static_cast<int32_t>(B / 4 + 2),
                                       device, &parser_),
           "ffm_engine_textparse_create");
  const int rc = ffm_engine_rowcut_create(static_cast<int32_t>(max_rows_), static_cast<int32_t>(max_nnz_), kRing, device, &cutter_);
  if (rc != FFM_OK) {
    ffm_engine_textparse_destroy(parser_);
    check_rc(rc, "ffm_engine_rowcut_create");
  }
}

RowStream::~RowStream() {
  if (reading_) read_.wait();
  ffm_engine_rowcut_destroy(cutter_);  // (waits for the device: the takes read the parser's slots)
  ffm_engine_textparse_destroy(parser_);
}

void RowStream::start_parse(Chunk &c) {
  chunks_++;
  bytes_ += c.text.n_bytes;
  if (c.text.host_only) return;
  check_rc(ffm_engine_textparse_parse(parser_, c.text.slot, c.text.data, static_cast<int64_t>(c.text.n_bytes), c.text.pinned ? 1 : 0),
           "ffm_engine_textparse_parse");
  c.started = true;
}

bool RowStream::fetch(Chunk &c) {
  c.started = c.ready = c.on_device = false;
  c.mirror = nullptr;
  if (!text_.next(&c.text)) return false;
  start_parse(c);
  return true;
}

void RowStream::begin_read(Chunk &c) {
  c.started = c.ready = c.on_device = false;
  c.mirror = nullptr;
  reading_ = &c;
  read_ = std::async(std::launch::async, [this, &c] { return text_.next(&c.text); });
}

void RowStream::finish_read(bool wait) {
  if (!reading_) return;
  if (!wait && read_.wait_for(std::chrono::seconds(0)) != std::future_status::ready) return;
  Chunk &c = *reading_;
  reading_ = nullptr;
  have_next_ = read_.get();  // (a failed read throws here, on the caller's thread)
  if (have_next_) start_parse(c);
}

void RowStream::make_ready(Chunk &c) {
  unsigned long long first_byte = c.text.file_offset;
  if (c.started) {
    ffm_text_block blk{};
    const int32_t *mirror = nullptr;
    check_rc(ffm_engine_textparse_wait_rows(parser_, c.text.slot, &blk, &mirror), "ffm_engine_textparse_wait_rows");
    c.started = false;
    if (blk.n_slow == 0 && !blk.overflow) {
      c.on_device = true;
      c.mirror = mirror;
      c.cut.row_ptr = mirror;
      c.cut.n_rows = static_cast<size_t>(blk.n_rows);
      c.ready = true;
      return;
    }
    if (blk.n_slow > 0) first_byte += static_cast<unsigned long long>(blk.first_slow_byte);
  }
  // the host parser's, whole (a malformed line: `wrong input: ...`, std::out_of_range)
  if (by_host_++ == 0) first_host_ = first_byte;
  c.part.clear();
  parse_csr_range(c.text.data, c.text.data + c.text.n_bytes, has_field_, c.part);
  c.row_ptr.resize(c.part.nnz.size() + 1);
  c.row_ptr[0] = 0;
  for (size_t r = 0; r < c.part.nnz.size(); r++) c.row_ptr[r + 1] = c.row_ptr[r] + c.part.nnz[r];
  c.cut.row_ptr = c.row_ptr.data();
  c.cut.n_rows = c.part.nnz.size();
  c.ready = true;
}

const RowCutChunk *RowStream::chunk_at(size_t ordinal) {
  if (!begun_) {  // chunk 0, and chunk 1 read behind it
    begun_ = true;
    cur_ord_ = 0;
    have_cur_ = fetch(chunk_[0]);
    have_next_ = false;
    if (have_cur_) begin_read(chunk_[1]);
  }
  while (ordinal > cur_ord_) {
    if (!have_cur_) return nullptr;
    // every row of the chunk has been taken (on the parser's stream): its slot takes the chunk after the next
    finish_read(true);
    cur_ord_++;
    have_cur_ = have_next_;
    have_next_ = false;
    if (have_cur_) begin_read(chunk_[(cur_ord_ + 1) & 1]);
  }
  if (!have_cur_) return nullptr;
  finish_read(false);  // (the next chunk's parse goes to the device as soon as its bytes are read)
  Chunk &c = chunk_[cur_ord_ & 1];
  if (!c.ready) make_ready(c);
  return &c.cut;
}

void RowStream::take(const RowSegment &seg) {
  Chunk &c = chunk_[seg.chunk & 1];
  if (c.on_device) {
    check_rc(ffm_engine_rowcut_take(cutter_, parser_, c.text.slot, static_cast<int32_t>(seg.r0), static_cast<int32_t>(seg.r1)),
             "ffm_engine_rowcut_take");
    return;
  }
  const size_t e0 = static_cast<size_t>(c.row_ptr[seg.r0]);
  check_rc(ffm_engine_rowcut_take_host(cutter_, static_cast<int32_t>(seg.r1 - seg.r0), c.row_ptr.data() + seg.r0, c.part.field.data() + e0,
                                       c.part.feat.data() + e0, c.part.val.data() + e0, c.part.label.data() + seg.r0),
           "ffm_engine_rowcut_take_host");
}

size_t RowStream::next(size_t want, ffm_rows_block *out) {
  const int idx = ring_pos_;
  if (held_[idx]) {  // the block that lived there must have been pulled
    while (pulled_() < seq_[idx]) std::this_thread::yield();
    check_rc(ffm_engine_rowcut_release(cutter_, idx), "ffm_engine_rowcut_release");
    held_[idx] = false;
  }
  const size_t got = plan_block(
      std::min(want, max_rows_), max_nnz_, true, cursor_, [&](size_t ordinal) { return chunk_at(ordinal); },
      [&](const RowSegment &seg) { take(seg); });
  if (got == 0) return 0;
  check_rc(ffm_engine_rowcut_close(cutter_, out), "ffm_engine_rowcut_close");
  held_[idx] = true;
  seq_[idx] = 0;
  ring_pos_ = (idx + 1) % kRing;
  blocks_++;
  return got;
}

void RowStream::rewind() {
  finish_read(true);
  for (Chunk &c : chunk_)
    if (c.started) {  // (a pass that ended early: nothing may stay in flight)
      ffm_text_block blk{};
      check_rc(ffm_engine_textparse_wait(parser_, c.text.slot, &blk), "ffm_engine_textparse_wait");
      c.started = false;
    }
  if (by_host_)
    std::printf("device rows: %s %llu chunks, %llu bytes, %llu parsed by the host (first at byte %llu), %llu blocks\n", pass_.c_str(), chunks_,
                bytes_, by_host_, first_host_, blocks_);
  else
    std::printf("device rows: %s %llu chunks, %llu bytes, 0 parsed by the host, %llu blocks\n", pass_.c_str(), chunks_, bytes_, blocks_);
  text_.rewind();
  begun_ = have_cur_ = have_next_ = false;
  cur_ord_ = 0;
  cursor_ = RowCutCursor{};
  chunks_ = bytes_ = by_host_ = first_host_ = blocks_ = 0;
}

}  // namespace ftrl
