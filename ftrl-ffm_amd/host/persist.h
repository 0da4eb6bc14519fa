// persist.h -- model files in the reference's formats (reference src/model/ffm.cpp:138-200,
// src/model/lr.cpp:26-39, src/compression/compress.cpp:15-51), plus a sidecar for the FTRL
// accumulators so that a checkpoint is actually resumable (the reference saves only w, and its
// first train() after a load recomputes w from zero (n,z)).
//
//   text        : "bias\n", n_feats lines of lin_w, n_feats lines of row_len space-separated floats
//   compressed  : ONE zstd frame holding float32 [bias, lin_w[n_feats], vec_w row-major]
//   state (.nz) : one zstd frame of float32 [bias_n, bias_z, lin_n[], lin_z[], vec_n[], vec_z[]]
//   sparse checkpoint : a fixed little-endian header, then one zstd frame holding only the records
//                 that differ from a freshly created model (SparseCheckpointWriter below)
//
// Everything streams: a writer takes the floats chunk by chunk (the model hands over a few tens of
// thousands of records at a time, pulled from HBM with ffm_engine_get_rows), a reader hands them
// back chunk by chunk -- the 33 M-feature headline model is 82 GB of w, which no host vector holds.
// The compressed frame is produced with zstd's streaming API and a pledged source size, so its
// header carries the content size the reference's one-shot loader asks for (ZSTD_getFrameContentSize,
// compress.cpp:33-40): files interchange both ways.
//
// zstd is taken from the system's libzstd.so.1 at run time (dlopen); if it is absent the compressed
// calls throw std::runtime_error and the text format still works.
#pragma once
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

namespace ftrl {

bool zstd_available();

// One zstd frame of `total_floats` float32 values, fed in any number of pieces.
class FloatFrameWriter {
 public:
  // `prefix`: bytes written to the file as they are, ahead of the frame (a header)
  FloatFrameWriter(const std::string &path, size_t total_floats, int level, const std::string &prefix = std::string());
  ~FloatFrameWriter();
  void write(const float *p, size_t n);
  void finish();  // flushes the frame; prints the reference's "saving to ..." line

 private:
  struct Impl;
  std::unique_ptr<Impl> d_;
};

// Reads such a frame (streaming or one-shot made) piece by piece.
class FloatFrameReader {
 public:
  // `offset`: where in the file the frame starts (behind a header)
  explicit FloatFrameReader(const std::string &path, size_t offset = 0);
  ~FloatFrameReader();
  size_t total_floats() const;        // from the frame header
  size_t read(float *p, size_t n);    // up to n floats; 0 at the end of the frame

 private:
  struct Impl;
  std::unique_ptr<Impl> d_;
};

// ---- sparse checkpoint ---------------------------------------------------------------------------
// A freshly created model is a pure function of (shape, seed, init_mean, init_stddev, flags), so a
// checkpoint needs only the features that no longer hold their create-time state (the engine lists
// them: ffm_engine_changed_features) -- a few per cent of the headline model after millions of rows,
// where the dense pair above is 247 GB.  File: 8 bytes of magic, a 32-bit version, the fields of the
// header below in their order (little-endian; 4 bytes of padding behind the bias: kSparseHeaderBytes),
// then ONE zstd frame of 32-bit words:
//   ids[n_changed]  (int32 patterns, strictly ascending, inside [0, n_feats))
//   then the records in chunks of `chunk` features (the last one shorter), per chunk of c features:
//   lin_w[c] lin_n[c] lin_z[c] vec_w[c * row_len] vec_n[c * row_len] vec_z[c * row_len]
// = n_changed * (4 + 3 * row_len) words, which the frame header's content size must match.
// Nothing here knows the engine: the pair is tested alone.
struct SparseCheckpointHeader {
  int32_t model_type = 0, n_feats = 0, n_fields = 0, n_factors = 0;
  uint32_t flags = 0;           // FFM_FLAG_* the model was created with
  int64_t row_len = 0;          // floats per latent component of a record (0: LR)
  uint64_t seed = 0;
  uint32_t init_mean_bits = 0, init_stddev_bits = 0;  // the floats' bit patterns
  int64_t n_changed = 0;
  int64_t chunk = 1;            // features per record chunk of the body
  uint32_t bias_bits[3] = {0, 0, 0};  // bias, bias_n, bias_z
  int64_t rows_seen = 0, epochs_done = 0;  // trainer progress (block-size ramp, shuffle sequence)
};
constexpr size_t kSparseHeaderBytes = 104;
constexpr uint32_t kSparseVersion = 1;

class SparseCheckpointWriter {
 public:
  // `ids`: h.n_changed ascending feature ids (checked).  Throws std::invalid_argument on a bad header.
  SparseCheckpointWriter(const std::string &path, const SparseCheckpointHeader &h, const int32_t *ids, int level);
  ~SparseCheckpointWriter();
  // the records of the next c ids, c = min(h.chunk, what is left); vec_* may be null when row_len == 0
  void chunk(size_t c, const float *lin_w, const float *lin_n, const float *lin_z, const float *vec_w,
             const float *vec_n, const float *vec_z);
  void finish();

 private:
  SparseCheckpointHeader h_;
  std::unique_ptr<FloatFrameWriter> w_;
  size_t done_ = 0;
};

class SparseCheckpointReader {
 public:
  // Reads and checks the header and the ids; throws std::runtime_error on a wrong magic or version, a
  // truncated file, a body whose length does not match the header, ids not strictly ascending or
  // outside [0, n_feats).
  explicit SparseCheckpointReader(const std::string &path);
  ~SparseCheckpointReader();
  const SparseCheckpointHeader &header() const { return h_; }
  const std::vector<int32_t> &ids() const { return ids_; }
  size_t next_chunk_size() const;  // 0 when every record has been read
  void chunk(float *lin_w, float *lin_n, float *lin_z, float *vec_w, float *vec_n, float *vec_z);
  void finish();  // the frame must end here

 private:
  std::string path_;
  SparseCheckpointHeader h_;
  std::vector<int32_t> ids_;
  std::unique_ptr<FloatFrameReader> r_;
  size_t done_ = 0;
  void need(float *p, size_t n);
};

// The text format, line by line (ffm.cpp:163-200).
class TextModelWriter {
 public:
  explicit TextModelWriter(const std::string &path);
  void scalar(float v);                               // "bias\n" / one lin_w line: ostream default precision
  void rows(const float *p, size_t n_rows, size_t row_len);  // shortest round-trip floats, space separated
  void finish();

 private:
  std::ofstream f_;
  std::string path_;
};
class TextModelReader {
 public:
  explicit TextModelReader(const std::string &path);
  float scalar();
  void rows(float *p, size_t n_rows, size_t row_len);

 private:
  std::ifstream f_;
  std::string path_, line_;
};

}  // namespace ftrl
