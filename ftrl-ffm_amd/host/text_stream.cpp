#include "text_stream.h"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <thread>

namespace ftrl {

namespace {

void check_rc(int rc, const char *what) {
  if (rc != FFM_OK) throw std::runtime_error(std::string(what) + ": " + ffm_engine_last_error());
}

void pread_all(int fd, char *dst, size_t n, unsigned long long off) {
  while (n > 0) {
    const ssize_t got = ::pread(fd, dst, n, static_cast<off_t>(off));
    if (got < 0 && errno == EINTR) continue;
    if (got <= 0) throw std::runtime_error("reading the training file failed");
    dst += got;
    off += static_cast<unsigned long long>(got);
    n -= static_cast<size_t>(got);
  }
}

struct ParserHandle {
  ffm_textparse *p = nullptr;
  ~ParserHandle() { ffm_engine_textparse_destroy(p); }
};

}  // namespace

TextChunkStream::TextChunkStream(const std::string &path, int n_threads, size_t slot_bytes)
    : n_threads_(std::max(1, std::min(n_threads, 8))), slot_bytes_((std::max<size_t>(slot_bytes, 16) + 4095) & ~static_cast<size_t>(4095)) {
  fd_ = ::open(path.c_str(), O_RDONLY);
  struct stat st {};
  if (fd_ < 0 || fstat(fd_, &st) != 0) {
    std::cerr << "fail to open " << path << std::endl;
    std::exit(EXIT_FAILURE);
  }
  size_ = static_cast<unsigned long long>(st.st_size);
  for (int s = 0; s < 2; s++) {
    slot_[s] = static_cast<char *>(std::aligned_alloc(4096, slot_bytes_));
    if (!slot_[s]) throw std::bad_alloc();
    // (no page-locked memory to be had: the parser copies each chunk into its own)
    pinned_[s] = ffm_engine_pin_host(slot_[s], slot_bytes_) == FFM_OK;
  }
}

TextChunkStream::~TextChunkStream() {
  for (int s = 0; s < 2; s++) {
    if (pinned_[s]) ffm_engine_unpin_host(slot_[s]);
    std::free(slot_[s]);
  }
  if (fd_ >= 0) ::close(fd_);
}

void TextChunkStream::read_at(char *dst, size_t n, unsigned long long off) {
  const size_t piece = std::max<size_t>((n + static_cast<size_t>(n_threads_) - 1) / static_cast<size_t>(n_threads_), 1 << 20);
  if (n <= piece) {
    pread_all(fd_, dst, n, off);
    return;
  }
  std::vector<std::thread> helpers;
  std::vector<int> failed((n + piece - 1) / piece, 0);
  for (size_t at = piece, k = 1; at < n; at += piece, k++)
    helpers.emplace_back([=, &failed] {
      try {
        pread_all(fd_, dst + at, std::min(piece, n - at), off + at);
      } catch (const std::exception &) {
        failed[k] = 1;
      }
    });
  try {
    pread_all(fd_, dst, piece, off);
  } catch (const std::exception &) {
    failed[0] = 1;
  }
  for (auto &t : helpers) t.join();
  if (std::find(failed.begin(), failed.end(), 1) != failed.end()) throw std::runtime_error("reading the training file failed");
}

bool TextChunkStream::next(TextChunk *out) {
  if (pos_ >= size_ && tail_len_ == 0) return false;
  const int s = turn_;
  turn_ ^= 1;
  char *buf = slot_[s];
  const unsigned long long chunk_off = pos_ - tail_len_;
  size_t have = tail_len_;
  if (have) std::memcpy(buf, tail_, have);  // (the tail lies in the other slot)
  tail_ = nullptr;
  tail_len_ = 0;
  const size_t want = static_cast<size_t>(std::min<unsigned long long>(slot_bytes_ - have, size_ - pos_));
  if (want) read_at(buf + have, want, pos_);
  pos_ += want;
  have += want;
  out->file_offset = chunk_off;
  out->slot = s;
  out->pinned = pinned_[s];
  out->host_only = false;
  out->data = buf;
  if (pos_ >= size_) {  // the end of the file: everything, a last line without its '\n' included
    out->n_bytes = have;
    return true;
  }
  size_t cut = have;
  while (cut > 0 && buf[cut - 1] != '\n') cut--;
  if (cut > 0) {
    out->n_bytes = cut;
    tail_ = buf + cut;
    tail_len_ = have - cut;
    return true;
  }
  // a single line longer than a slot: all of it, up to its '\n' or the file's end, for the host parser
  std::vector<char> &long_line = long_line_[s];  // (one per slot: the chunk before this one may be such a line too)
  long_line.assign(buf, buf + have);
  std::vector<char> more(1 << 20);
  bool ended = false;
  while (!ended && pos_ < size_) {
    const size_t n = static_cast<size_t>(std::min<unsigned long long>(more.size(), size_ - pos_));
    pread_all(fd_, more.data(), n, pos_);
    const void *nl = std::memchr(more.data(), '\n', n);
    const size_t take = nl ? static_cast<size_t>(static_cast<const char *>(nl) - more.data()) + 1 : n;
    long_line.insert(long_line.end(), more.begin(), more.begin() + static_cast<std::ptrdiff_t>(take));
    pos_ += take;
    ended = nl != nullptr;
  }
  out->data = long_line.data();
  out->n_bytes = long_line.size();
  out->pinned = false;
  out->host_only = true;
  return true;
}

void TextChunkStream::rewind() {
  pos_ = 0;
  tail_ = nullptr;
  tail_len_ = 0;
  turn_ = 0;
}

size_t TextChunkStream::slot_bytes_from_env() {
  const char *slot_env = std::getenv("FFM_TEXT_SLOT_BYTES");
  const long long slot_bytes = slot_env ? std::atoll(slot_env) : 0;
  return slot_bytes >= 16 && slot_bytes <= (1ll << 30) ? static_cast<size_t>(slot_bytes) : kSlotBytes;
}

unsigned long long device_parse_pass(const config_options &opt, const DeviceParseHooks &hooks) {
  const bool has_field = opt.file_type == "libffm";
  TextChunkStream ts(opt.train_path, opt.thread_num, TextChunkStream::slot_bytes_from_env());
  ParserHandle tp;
  {
    // capacities no chunk can exceed: a row is at least 2 bytes of text ("1\n"), an entry at least 4 ("1:1 ")
    const size_t B = ts.slot_bytes();
    check_rc(ffm_engine_textparse_create(has_field ? 1 : 0, static_cast<int64_t>(B), static_cast<int32_t>(B / 2 + 1),
                                         static_cast<int32_t>(B / 4 + 2), opt.device, &tp.p),
             "ffm_engine_textparse_create");
  }
  unsigned long long rows = 0, chunks = 0, bytes = 0, by_host = 0, first_host = 0;
  CsrPart part;
  auto on_host = [&](const TextChunk &c, unsigned long long first_byte) {
    if (by_host++ == 0) first_host = first_byte;
    part.clear();
    parse_csr_range(c.data, c.data + c.n_bytes, has_field, part);  // (a malformed line: `wrong input: ...`, std::out_of_range)
    rows += part.nnz.size();
    hooks.host(part);
  };
  auto start = [&](const TextChunk &c) {
    if (c.host_only) return;
    hooks.sync();  // (the slot's arrays were handed to the counting object two chunks ago)
    check_rc(ffm_engine_textparse_parse(tp.p, c.slot, c.data, static_cast<int64_t>(c.n_bytes), c.pinned ? 1 : 0), "ffm_engine_textparse_parse");
  };
  TextChunk cur, nxt;
  bool have = ts.next(&cur);
  if (have) start(cur);
  while (have) {
    const bool have_next = ts.next(&nxt);  // (into the other slot, while the device parses this one)
    if (have_next) start(nxt);
    chunks++;
    bytes += cur.n_bytes;
    if (cur.host_only) {
      on_host(cur, cur.file_offset);
    } else {
      ffm_text_block blk{};
      check_rc(ffm_engine_textparse_wait(tp.p, cur.slot, &blk), "ffm_engine_textparse_wait");
      if (blk.n_slow > 0 || blk.overflow) {
        on_host(cur, cur.file_offset + static_cast<unsigned long long>(blk.n_slow > 0 ? blk.first_slow_byte : 0));
      } else {
        rows += static_cast<unsigned long long>(blk.n_rows);
        hooks.device(blk);
      }
    }
    cur = nxt;
    have = have_next;
  }
  hooks.sync();  // (before the parser and its arrays go)
  if (by_host)
    std::printf("device parse: %llu chunks, %llu bytes, %llu parsed by the host (first at byte %llu)\n", chunks, bytes, by_host, first_host);
  else
    std::printf("device parse: %llu chunks, %llu bytes, 0 parsed by the host\n", chunks, bytes);
  return rows;
}

}  // namespace ftrl
