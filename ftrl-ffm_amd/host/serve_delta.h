// serve_delta.h -- the serving delta file: what one ffm_engine_sync_weights moved in a serving engine, in the
// table's own bits (include/ffm_engine.h "Serving deltas").  Delta number seq turns the serving model that has
// applied deltas 1 .. seq - 1 into the one the trainer published as seq; delta 1 is relative to a fresh serving
// engine's create-time contents, which is why the header carries the seed and the init distribution.
//
// File: 8 bytes of magic, a 32-bit version, the fields of the header below (little-endian, the 64-bit ones on
// 8-byte offsets: kServeDeltaHeaderBytes), then ONE zstd frame of 32-bit words:
//   ids[n_moved]  (int32 patterns, strictly ascending, inside [0, n_feats))
//   then the rows in chunks of `chunk` features (the last one shorter), per chunk of c features:
//   lin_w[c] (fp32 patterns), then the c rows' raw bits: c * row_len words for f32, c * row_len / 2 for f16
// = n_moved * (2 + row_words) words, which the frame header's content size must match.
// Nothing here knows the engine, like the sparse checkpoint pair of persist.h whose frames it reuses.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "persist.h"

namespace ftrl {

enum { kServeDeltaF32 = 1, kServeDeltaF16 = 2 };

struct ServeDeltaHeader {
  int32_t model_type = 0, n_feats = 0, n_fields = 0, n_factors = 0;
  uint32_t hash_ids = 0;        // 1: the model was created with FFM_FLAG_HASH_IDS
  uint32_t format = 0;          // kServeDeltaF32 / kServeDeltaF16
  int64_t row_len = 0;          // elements of a row
  uint64_t seed = 0;
  uint32_t init_mean_bits = 0, init_stddev_bits = 0;  // the floats' bit patterns
  int64_t seq = 0;              // 1-based
  int64_t n_moved = 0;
  int64_t chunk = 1;            // features per chunk of the body
  uint32_t bias_bits = 0;
  // 32-bit words of one row in the body
  size_t row_words() const { return static_cast<size_t>(format == kServeDeltaF16 ? row_len / 2 : row_len); }
  size_t body_words() const { return static_cast<size_t>(n_moved) * (2 + row_words()); }
};
constexpr size_t kServeDeltaHeaderBytes = 96;
constexpr uint32_t kServeDeltaVersion = 1;

class ServeDeltaWriter {
 public:
  // `ids`: h.n_moved ascending feature ids (checked).  Throws std::invalid_argument on a bad header.
  ServeDeltaWriter(const std::string &path, const ServeDeltaHeader &h, const int32_t *ids, int level);
  ~ServeDeltaWriter();
  // the next c ids' lin_w and raw rows ([c][row_len] elements of 4 or 2 bytes), c = min(h.chunk, what is left)
  void chunk(size_t c, const float *lin_w, const void *lat);
  void finish();
  size_t bytes_in() const { return kServeDeltaHeaderBytes + 4 * h_.body_words(); }  // header + uncompressed body

 private:
  ServeDeltaHeader h_;
  std::unique_ptr<FloatFrameWriter> w_;
  size_t done_ = 0;
};

class ServeDeltaReader {
 public:
  // Reads and checks the header and the ids; throws std::runtime_error, with the path in the message, on a wrong
  // magic or version, a truncated file, a body whose length does not match the header, ids not strictly
  // ascending or outside [0, n_feats).
  explicit ServeDeltaReader(const std::string &path);
  ~ServeDeltaReader();
  const ServeDeltaHeader &header() const { return h_; }
  const std::vector<int32_t> &ids() const { return ids_; }
  size_t next_chunk_size() const;  // 0 when every row has been read
  void chunk(float *lin_w, void *lat);
  void finish();  // the frame must end here

 private:
  std::string path_;
  ServeDeltaHeader h_;
  std::vector<int32_t> ids_;
  std::unique_ptr<FloatFrameReader> r_;
  size_t done_ = 0;
  void need(float *p, size_t n);
};

// The header alone (magic, version, fields; nothing of the frame): what a command line checks before a device
// is opened.  Throws like the reader.
ServeDeltaHeader read_serve_delta_header(const std::string &path);

}  // namespace ftrl
