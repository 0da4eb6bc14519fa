// serve_delta.cpp -- the serving delta file (serve_delta.h): a fixed little-endian header and one zstd frame.
#include "serve_delta.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <stdexcept>

namespace ftrl {

namespace {
const char kDeltaMagic[8] = {'F', 'F', 'M', 'S', 'D', 'L', 'T', '\n'};

void put_le(std::string &out, uint64_t v, int bytes) {
  for (int i = 0; i < bytes; i++) out.push_back(static_cast<char>((v >> (8 * i)) & 0xff));
}
uint64_t get_le(const unsigned char *&p, int bytes) {
  uint64_t v = 0;
  for (int i = 0; i < bytes; i++) v |= static_cast<uint64_t>(p[i]) << (8 * i);
  p += bytes;
  return v;
}
std::string pack_header(const ServeDeltaHeader &h) {
  std::string out(kDeltaMagic, sizeof kDeltaMagic);
  put_le(out, kServeDeltaVersion, 4);
  put_le(out, static_cast<uint32_t>(h.model_type), 4);
  put_le(out, static_cast<uint32_t>(h.n_feats), 4);
  put_le(out, static_cast<uint32_t>(h.n_fields), 4);
  put_le(out, static_cast<uint32_t>(h.n_factors), 4);
  put_le(out, h.hash_ids, 4);
  put_le(out, h.format, 4);
  put_le(out, 0, 4);  // (padding: the 64-bit fields sit on 8-byte offsets)
  put_le(out, static_cast<uint64_t>(h.row_len), 8);
  put_le(out, h.seed, 8);
  put_le(out, h.init_mean_bits, 4);
  put_le(out, h.init_stddev_bits, 4);
  put_le(out, static_cast<uint64_t>(h.seq), 8);
  put_le(out, static_cast<uint64_t>(h.n_moved), 8);
  put_le(out, static_cast<uint64_t>(h.chunk), 8);
  put_le(out, h.bias_bits, 4);
  put_le(out, 0, 4);
  return out;
}
bool consistent(const ServeDeltaHeader &h) {
  return h.n_feats > 0 && (h.format == kServeDeltaF32 || h.format == kServeDeltaF16) && h.row_len >= 0 &&
         h.row_len <= (1ll << 32) && !(h.format == kServeDeltaF16 && h.row_len % 2 != 0) && h.seq >= 1 && h.n_moved >= 0 &&
         h.n_moved <= h.n_feats && h.chunk > 0 && h.hash_ids <= 1;
}
// int32 ids, fp32 patterns and packed halves share the frame as 32-bit words
const float *as_words(const void *p) { return static_cast<const float *>(p); }
}  // namespace

ServeDeltaWriter::ServeDeltaWriter(const std::string &path, const ServeDeltaHeader &h, const int32_t *ids, int level) : h_(h) {
  if (!consistent(h)) throw std::invalid_argument("ServeDeltaWriter: bad header");
  for (int64_t j = 0; j < h.n_moved; j++)
    if (ids[j] < 0 || ids[j] >= h.n_feats || (j > 0 && ids[j] <= ids[j - 1]))
      throw std::invalid_argument("ServeDeltaWriter: ids must ascend strictly inside [0, n_feats)");
  const std::string head = pack_header(h);
  if (head.size() != kServeDeltaHeaderBytes) throw std::logic_error("ServeDeltaWriter: header size");
  w_ = std::make_unique<FloatFrameWriter>(path, h.body_words(), level, head);
  if (h.n_moved) w_->write(as_words(ids), static_cast<size_t>(h.n_moved));
}
ServeDeltaWriter::~ServeDeltaWriter() = default;
void ServeDeltaWriter::chunk(size_t c, const float *lin_w, const void *lat) {
  const size_t left = static_cast<size_t>(h_.n_moved) - done_, rw = h_.row_words();
  if (c == 0 || c != std::min(left, static_cast<size_t>(h_.chunk)))
    throw std::logic_error("ServeDeltaWriter: a chunk holds min(header.chunk, what is left) features");
  w_->write(lin_w, c);
  if (rw) w_->write(as_words(lat), c * rw);
  done_ += c;
}
void ServeDeltaWriter::finish() {
  if (done_ != static_cast<size_t>(h_.n_moved)) throw std::logic_error("ServeDeltaWriter: rows missing");
  w_->finish();
}

ServeDeltaHeader read_serve_delta_header(const std::string &path) {
  unsigned char raw[kServeDeltaHeaderBytes];
  {
    std::FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("Failed to open loading file " + path);
    const size_t got = std::fread(raw, 1, sizeof raw, f);
    std::fclose(f);
    if (got < sizeof kDeltaMagic || std::memcmp(raw, kDeltaMagic, sizeof kDeltaMagic) != 0)
      throw std::runtime_error(path + ": not a serving delta (wrong magic)");
    if (got != sizeof raw) throw std::runtime_error(path + ": serving delta header is truncated");
  }
  const unsigned char *p = raw + sizeof kDeltaMagic;
  const uint32_t version = static_cast<uint32_t>(get_le(p, 4));
  if (version != kServeDeltaVersion)
    throw std::runtime_error(path + ": serving delta version " + std::to_string(version) + ", this build reads " +
                             std::to_string(kServeDeltaVersion));
  ServeDeltaHeader h;
  h.model_type = static_cast<int32_t>(get_le(p, 4));
  h.n_feats = static_cast<int32_t>(get_le(p, 4));
  h.n_fields = static_cast<int32_t>(get_le(p, 4));
  h.n_factors = static_cast<int32_t>(get_le(p, 4));
  h.hash_ids = static_cast<uint32_t>(get_le(p, 4));
  h.format = static_cast<uint32_t>(get_le(p, 4));
  (void)get_le(p, 4);
  h.row_len = static_cast<int64_t>(get_le(p, 8));
  h.seed = get_le(p, 8);
  h.init_mean_bits = static_cast<uint32_t>(get_le(p, 4));
  h.init_stddev_bits = static_cast<uint32_t>(get_le(p, 4));
  h.seq = static_cast<int64_t>(get_le(p, 8));
  h.n_moved = static_cast<int64_t>(get_le(p, 8));
  h.chunk = static_cast<int64_t>(get_le(p, 8));
  h.bias_bits = static_cast<uint32_t>(get_le(p, 4));
  if (!consistent(h)) throw std::runtime_error(path + ": serving delta header is inconsistent");
  return h;
}

ServeDeltaReader::ServeDeltaReader(const std::string &path) : path_(path), h_(read_serve_delta_header(path)) {
  r_ = std::make_unique<FloatFrameReader>(path, kServeDeltaHeaderBytes);
  if (r_->total_floats() != h_.body_words())
    throw std::runtime_error(path + ": body length does not match the header (" + std::to_string(r_->total_floats()) +
                             " words, header implies " + std::to_string(h_.body_words()) + ")");
  ids_.resize(static_cast<size_t>(h_.n_moved));
  need(reinterpret_cast<float *>(ids_.data()), ids_.size());
  for (size_t j = 0; j < ids_.size(); j++)
    if (ids_[j] < 0 || ids_[j] >= h_.n_feats || (j > 0 && ids_[j] <= ids_[j - 1]))
      throw std::runtime_error(path + ": feature ids must ascend strictly inside [0, n_feats)");
}
ServeDeltaReader::~ServeDeltaReader() = default;
void ServeDeltaReader::need(float *p, size_t n) {
  if (n && r_->read(p, n) != n) throw std::runtime_error(path_ + ": zstd frame is truncated");
}
size_t ServeDeltaReader::next_chunk_size() const {
  return std::min(static_cast<size_t>(h_.n_moved) - done_, static_cast<size_t>(h_.chunk));
}
void ServeDeltaReader::chunk(float *lin_w, void *lat) {
  const size_t c = next_chunk_size(), rw = h_.row_words();
  need(lin_w, c);
  if (rw) need(static_cast<float *>(lat), c * rw);
  done_ += c;
}
void ServeDeltaReader::finish() {
  if (next_chunk_size() != 0) throw std::logic_error("ServeDeltaReader: rows left unread");
  float extra;
  if (r_->read(&extra, 1) != 0) throw std::runtime_error(path_ + ": body is longer than the header implies");
}

}  // namespace ftrl
