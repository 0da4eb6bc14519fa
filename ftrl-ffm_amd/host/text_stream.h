// text_stream.h -- --device_parse true: the training file as a stream of RAW TEXT chunks in file order, and the loop
// a counting pre-pass (field_count.cpp, rare_count.cpp, value_count.cpp) runs over them.  The host does nothing per
// byte but copy it: pread fills one of two page-locked slots, the slot is cut at its last '\n' and the tail carried
// into the next one, and the device parses the bytes (ffm_textparse, include/ffm_engine.h "Text blocks") into the
// arrays the pass's *_add_device entry point takes.  A chunk the device will not parse -- a line outside its grammar,
// a single line longer than a slot -- goes through parse_csr_range on the host, whole, and is handed over the way
// the pass hands over blocks without the flag: so a malformed line prints the same `wrong input: ...` and the run
// ends the same way.
#pragma once
#include <functional>
#include <string>
#include <vector>

#include "cmd_option.h"
#include "count_block.h"

namespace ftrl {

struct TextChunk {
  const char *data = nullptr;  // whole lines (the file's last line may lack its '\n')
  size_t n_bytes = 0;
  unsigned long long file_offset = 0;
  int slot = 0;             // which of the two slots holds it (0 / 1, alternating)
  bool pinned = false;      // data is page-locked: the device may copy it by DMA
  bool host_only = false;   // a single line longer than a slot: not in a slot, the host parser's
};

class TextChunkStream {
 public:
  // a chunk is at most about kCountRows lines: a libffm row of 39 fields is about 550 bytes of text
  static constexpr size_t kSlotBytes = kCountRows * 640;
  TextChunkStream(const std::string &path, int n_threads, size_t slot_bytes = kSlotBytes);
  ~TextChunkStream();
  TextChunkStream(const TextChunkStream &) = delete;
  TextChunkStream &operator=(const TextChunkStream &) = delete;
  // The next chunk; false at the end of the file.  It stays valid until the call after the next one.
  bool next(TextChunk *out);
  size_t slot_bytes() const { return slot_bytes_; }
  void rewind();  // back to the file's first byte (the next pass); chunks handed out before are no longer valid
  // kSlotBytes, or what FFM_TEXT_SLOT_BYTES says: a TEST HOOK (`--device_parse true`), a test's way to many
  // chunks, carried tails and over-long lines from a small file; results do not depend on it
  static size_t slot_bytes_from_env();

 private:
  void read_at(char *dst, size_t n, unsigned long long off);  // pread by n_threads_ threads
  int fd_ = -1, n_threads_ = 1, turn_ = 0;
  unsigned long long size_ = 0, pos_ = 0;  // the file's size; the first byte not yet in a chunk or in the tail
  size_t slot_bytes_ = 0;
  char *slot_[2] = {nullptr, nullptr};
  bool pinned_[2] = {false, false};
  const char *tail_ = nullptr;  // the bytes behind the last chunk's last '\n', still in that chunk's slot
  size_t tail_len_ = 0;
  std::vector<char> long_line_[2];
};

// What a pass does with a chunk.
struct DeviceParseHooks {
  std::function<void(const ffm_text_block &)> device;  // the entries in HBM: *_add_device
  std::function<void(const CsrPart &)> host;           // a chunk the host parsed: *_add
  std::function<void()> sync;                          // back once the counting object has read what it was handed
};

// One pass over opt.train_path: every chunk parsed on the device (or, whole, on the host) and handed to the hooks in
// file order.  Returns the rows.  Prints `device parse: C chunks, B bytes, H parsed by the host (first at byte N)`.
unsigned long long device_parse_pass(const config_options &opt, const DeviceParseHooks &hooks);

}  // namespace ftrl
