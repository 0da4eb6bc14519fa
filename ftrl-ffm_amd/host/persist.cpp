#include "persist.h"

#include <dlfcn.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <stdexcept>

namespace ftrl {
namespace {

// libzstd entry points (the reference links the vendored library, compress.cpp:17-40), bound at run time.
struct ZInBuf { const void *src; size_t size; size_t pos; };
struct ZOutBuf { void *dst; size_t size; size_t pos; };
struct Zstd {
  void *(*createCCtx)() = nullptr;
  size_t (*freeCCtx)(void *) = nullptr;
  size_t (*cctxSetParameter)(void *, int, int) = nullptr;
  size_t (*cctxSetPledgedSrcSize)(void *, unsigned long long) = nullptr;
  size_t (*compressStream2)(void *, ZOutBuf *, ZInBuf *, int) = nullptr;
  void *(*createDCtx)() = nullptr;
  size_t (*freeDCtx)(void *) = nullptr;
  size_t (*decompressStream)(void *, ZOutBuf *, ZInBuf *) = nullptr;
  unsigned long long (*getFrameContentSize)(const void *, size_t) = nullptr;
  unsigned (*isError)(size_t) = nullptr;
  bool ok = false;
  Zstd() {
    void *h = dlopen("libzstd.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("libzstd.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) return;
#define BIND(field, sym) field = reinterpret_cast<decltype(field)>(dlsym(h, sym))
    BIND(createCCtx, "ZSTD_createCCtx");
    BIND(freeCCtx, "ZSTD_freeCCtx");
    BIND(cctxSetParameter, "ZSTD_CCtx_setParameter");
    BIND(cctxSetPledgedSrcSize, "ZSTD_CCtx_setPledgedSrcSize");
    BIND(compressStream2, "ZSTD_compressStream2");
    BIND(createDCtx, "ZSTD_createDCtx");
    BIND(freeDCtx, "ZSTD_freeDCtx");
    BIND(decompressStream, "ZSTD_decompressStream");
    BIND(getFrameContentSize, "ZSTD_getFrameContentSize");
    BIND(isError, "ZSTD_isError");
#undef BIND
    ok = createCCtx && freeCCtx && cctxSetParameter && cctxSetPledgedSrcSize && compressStream2 &&
         createDCtx && freeDCtx && decompressStream && getFrameContentSize && isError;
  }
};
Zstd &zstd() {
  static Zstd z;
  return z;
}
constexpr int kParamCompressionLevel = 100;  // ZSTD_c_compressionLevel
constexpr int kEndContinue = 0, kEndEnd = 2;  // ZSTD_e_continue / ZSTD_e_end
constexpr size_t kIoBuf = 1 << 20;

}  // namespace

bool zstd_available() { return zstd().ok; }

struct FloatFrameWriter::Impl {
  std::string path;      // the file as the caller named it
  std::string tmp_path;  // what is written: renamed over `path` by finish(), removed otherwise
  std::FILE *f = nullptr;
  void *cctx = nullptr;
  std::vector<char> out = std::vector<char>(kIoBuf);
  size_t total_bytes = 0, fed = 0, written = 0;
  bool done = false;
  void pump(const void *src, size_t bytes, int end_op) {
    ZInBuf in{src, bytes, 0};
    for (;;) {
      ZOutBuf ob{out.data(), out.size(), 0};
      const size_t r = zstd().compressStream2(cctx, &ob, &in, end_op);
      if (zstd().isError(r)) throw std::runtime_error("ZSTD_compressStream2 failed: " + path);
      if (ob.pos && std::fwrite(out.data(), 1, ob.pos, f) != ob.pos) throw std::runtime_error("cannot write " + path);
      written += ob.pos;
      if (end_op == kEndEnd ? r == 0 : in.pos == in.size) break;
    }
  }
};

FloatFrameWriter::FloatFrameWriter(const std::string &path, size_t total_floats, int level, const std::string &prefix)
    : d_(new Impl) {
  if (!zstd().ok) throw std::runtime_error("libzstd.so.1 not available");
  d_->path = path;
  d_->total_bytes = total_floats * sizeof(float);
  // written beside the target and renamed when complete: an exception half way (a device error while
  // the model is pulled, a full disk) leaves the previous checkpoint where it was
  d_->tmp_path = path + ".tmp";
  d_->f = std::fopen(d_->tmp_path.c_str(), "wb");
  if (!d_->f) throw std::runtime_error("cannot write " + d_->tmp_path);
  if (!prefix.empty() && std::fwrite(prefix.data(), 1, prefix.size(), d_->f) != prefix.size())
    throw std::runtime_error("cannot write " + d_->tmp_path);
  d_->cctx = zstd().createCCtx();
  if (!d_->cctx) throw std::runtime_error("ZSTD_createCCtx failed");
  if (zstd().isError(zstd().cctxSetParameter(d_->cctx, kParamCompressionLevel, level)))
    throw std::runtime_error("ZSTD_CCtx_setParameter(compressionLevel) failed");
  // the frame header then carries the content size, as a one-shot ZSTD_compress frame does -- this
  // reader and the reference's loader both need it there
  if (zstd().isError(zstd().cctxSetPledgedSrcSize(d_->cctx, d_->total_bytes)))
    throw std::runtime_error("ZSTD_CCtx_setPledgedSrcSize failed");
}
FloatFrameWriter::~FloatFrameWriter() {
  if (d_->cctx) zstd().freeCCtx(d_->cctx);
  if (d_->f) std::fclose(d_->f);
  if (!d_->done && !d_->tmp_path.empty()) std::remove(d_->tmp_path.c_str());  // an unfinished file
}
void FloatFrameWriter::write(const float *p, size_t n) {
  d_->fed += n * sizeof(float);
  if (d_->fed > d_->total_bytes) throw std::logic_error("FloatFrameWriter: more floats than pledged");
  d_->pump(p, n * sizeof(float), kEndContinue);
}
void FloatFrameWriter::finish() {
  if (d_->done) return;
  if (d_->fed != d_->total_bytes) throw std::logic_error("FloatFrameWriter: fewer floats than pledged");
  d_->pump(nullptr, 0, kEndEnd);
  const bool closed = std::fclose(d_->f) == 0;
  d_->f = nullptr;
  if (!closed || std::rename(d_->tmp_path.c_str(), d_->path.c_str()) != 0)
    throw std::runtime_error("cannot write " + d_->path);
  d_->done = true;
  std::printf("saving to %s, before: %zu -> after: %zu\n", d_->path.c_str(), d_->total_bytes, d_->written);
}

struct FloatFrameReader::Impl {
  std::string path;
  std::FILE *f = nullptr;
  void *dctx = nullptr;
  std::vector<char> in = std::vector<char>(kIoBuf);
  ZInBuf ib{nullptr, 0, 0};
  unsigned long long content = 0;
  bool frame_done = false;
  char carry[4];
  size_t n_carry = 0;  // bytes of a float split across two reads
};

FloatFrameReader::FloatFrameReader(const std::string &path, size_t offset) : d_(new Impl) {
  if (!zstd().ok) throw std::runtime_error("libzstd.so.1 not available");
  d_->path = path;
  d_->f = std::fopen(path.c_str(), "rb");
  if (!d_->f) throw std::runtime_error("Failed to open loading file " + path);
  if (offset && std::fseek(d_->f, static_cast<long>(offset), SEEK_SET) != 0)
    throw std::runtime_error(path + ": cannot seek to the frame");
  const size_t got = std::fread(d_->in.data(), 1, d_->in.size(), d_->f);
  d_->ib = ZInBuf{d_->in.data(), got, 0};
  d_->content = zstd().getFrameContentSize(d_->in.data(), got);
  if (d_->content == 0ULL - 1 || d_->content == 0ULL - 2)  // ZSTD_CONTENTSIZE_UNKNOWN / _ERROR
    throw std::runtime_error(path + ": not compressed by zstd!");
  d_->dctx = zstd().createDCtx();
}
FloatFrameReader::~FloatFrameReader() {
  if (d_->dctx) zstd().freeDCtx(d_->dctx);
  if (d_->f) std::fclose(d_->f);
}
size_t FloatFrameReader::total_floats() const { return static_cast<size_t>(d_->content / sizeof(float)); }
size_t FloatFrameReader::read(float *p, size_t n) {
  char *dst = reinterpret_cast<char *>(p);
  const size_t want = n * sizeof(float);
  size_t have = 0;
  if (d_->n_carry) { std::memcpy(dst, d_->carry, d_->n_carry); have = d_->n_carry; d_->n_carry = 0; }
  while (have < want && !d_->frame_done) {
    if (d_->ib.pos == d_->ib.size) {
      const size_t got = std::fread(d_->in.data(), 1, d_->in.size(), d_->f);
      if (got == 0) throw std::runtime_error(d_->path + ": zstd frame is truncated");
      d_->ib = ZInBuf{d_->in.data(), got, 0};
    }
    ZOutBuf ob{dst, want, have};
    const size_t r = zstd().decompressStream(d_->dctx, &ob, &d_->ib);
    if (zstd().isError(r)) throw std::runtime_error(d_->path + ": zstd frame is corrupt");
    have = ob.pos;
    if (r == 0) d_->frame_done = true;
  }
  const size_t whole = have / sizeof(float);
  d_->n_carry = have - whole * sizeof(float);
  if (d_->n_carry) std::memcpy(d_->carry, dst + whole * sizeof(float), d_->n_carry);
  return whole;
}

// ---- sparse checkpoint ---------------------------------------------------------------------------

namespace {
const char kSparseMagic[8] = {'F', 'F', 'M', 'S', 'P', 'C', 'K', '\n'};

void put_le(std::string &out, uint64_t v, int bytes) {
  for (int i = 0; i < bytes; i++) out.push_back(static_cast<char>((v >> (8 * i)) & 0xff));
}
uint64_t get_le(const unsigned char *&p, int bytes) {
  uint64_t v = 0;
  for (int i = 0; i < bytes; i++) v |= static_cast<uint64_t>(p[i]) << (8 * i);
  p += bytes;
  return v;
}
std::string pack_header(const SparseCheckpointHeader &h) {
  std::string out(kSparseMagic, sizeof kSparseMagic);
  put_le(out, kSparseVersion, 4);
  put_le(out, static_cast<uint32_t>(h.model_type), 4);
  put_le(out, static_cast<uint32_t>(h.n_feats), 4);
  put_le(out, static_cast<uint32_t>(h.n_fields), 4);
  put_le(out, static_cast<uint32_t>(h.n_factors), 4);
  put_le(out, h.flags, 4);
  put_le(out, static_cast<uint64_t>(h.row_len), 8);
  put_le(out, h.seed, 8);
  put_le(out, h.init_mean_bits, 4);
  put_le(out, h.init_stddev_bits, 4);
  put_le(out, static_cast<uint64_t>(h.n_changed), 8);
  put_le(out, static_cast<uint64_t>(h.chunk), 8);
  for (uint32_t b : h.bias_bits) put_le(out, b, 4);
  put_le(out, 0, 4);  // (padding: the 64-bit fields sit on 8-byte offsets)
  put_le(out, static_cast<uint64_t>(h.rows_seen), 8);
  put_le(out, static_cast<uint64_t>(h.epochs_done), 8);
  return out;
}
size_t body_words(const SparseCheckpointHeader &h) {
  return static_cast<size_t>(h.n_changed) * (4 + 3 * static_cast<size_t>(h.row_len));
}
// int32 ids and float records share the frame as 32-bit words
const float *as_words(const int32_t *p) { return reinterpret_cast<const float *>(p); }
}  // namespace

SparseCheckpointWriter::SparseCheckpointWriter(const std::string &path, const SparseCheckpointHeader &h,
                                               const int32_t *ids, int level)
    : h_(h) {
  if (h.n_feats <= 0 || h.row_len < 0 || h.n_changed < 0 || h.n_changed > h.n_feats || h.chunk <= 0)
    throw std::invalid_argument("SparseCheckpointWriter: bad header");
  for (int64_t j = 0; j < h.n_changed; j++)
    if (ids[j] < 0 || ids[j] >= h.n_feats || (j > 0 && ids[j] <= ids[j - 1]))
      throw std::invalid_argument("SparseCheckpointWriter: ids must ascend strictly inside [0, n_feats)");
  const std::string head = pack_header(h);
  if (head.size() != kSparseHeaderBytes) throw std::logic_error("SparseCheckpointWriter: header size");
  w_ = std::make_unique<FloatFrameWriter>(path, body_words(h), level, head);
  if (h.n_changed) w_->write(as_words(ids), static_cast<size_t>(h.n_changed));
}
SparseCheckpointWriter::~SparseCheckpointWriter() = default;
void SparseCheckpointWriter::chunk(size_t c, const float *lin_w, const float *lin_n, const float *lin_z,
                                   const float *vec_w, const float *vec_n, const float *vec_z) {
  const size_t left = static_cast<size_t>(h_.n_changed) - done_, rl = static_cast<size_t>(h_.row_len);
  if (c == 0 || c != std::min(left, static_cast<size_t>(h_.chunk)))
    throw std::logic_error("SparseCheckpointWriter: a chunk holds min(header.chunk, what is left) features");
  w_->write(lin_w, c);
  w_->write(lin_n, c);
  w_->write(lin_z, c);
  if (rl) {
    w_->write(vec_w, c * rl);
    w_->write(vec_n, c * rl);
    w_->write(vec_z, c * rl);
  }
  done_ += c;
}
void SparseCheckpointWriter::finish() { w_->finish(); }

SparseCheckpointReader::SparseCheckpointReader(const std::string &path) : path_(path) {
  unsigned char raw[kSparseHeaderBytes];
  {
    std::FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("Failed to open loading file " + path);
    const size_t got = std::fread(raw, 1, sizeof raw, f);
    std::fclose(f);
    if (got < sizeof kSparseMagic || std::memcmp(raw, kSparseMagic, sizeof kSparseMagic) != 0)
      throw std::runtime_error(path + ": not a sparse checkpoint (wrong magic)");
    if (got != sizeof raw) throw std::runtime_error(path + ": sparse checkpoint header is truncated");
  }
  const unsigned char *p = raw + sizeof kSparseMagic;
  const uint32_t version = static_cast<uint32_t>(get_le(p, 4));
  if (version != kSparseVersion)
    throw std::runtime_error(path + ": sparse checkpoint version " + std::to_string(version) + ", this build reads " + std::to_string(kSparseVersion));
  h_.model_type = static_cast<int32_t>(get_le(p, 4));
  h_.n_feats = static_cast<int32_t>(get_le(p, 4));
  h_.n_fields = static_cast<int32_t>(get_le(p, 4));
  h_.n_factors = static_cast<int32_t>(get_le(p, 4));
  h_.flags = static_cast<uint32_t>(get_le(p, 4));
  h_.row_len = static_cast<int64_t>(get_le(p, 8));
  h_.seed = get_le(p, 8);
  h_.init_mean_bits = static_cast<uint32_t>(get_le(p, 4));
  h_.init_stddev_bits = static_cast<uint32_t>(get_le(p, 4));
  h_.n_changed = static_cast<int64_t>(get_le(p, 8));
  h_.chunk = static_cast<int64_t>(get_le(p, 8));
  for (uint32_t &b : h_.bias_bits) b = static_cast<uint32_t>(get_le(p, 4));
  (void)get_le(p, 4);
  h_.rows_seen = static_cast<int64_t>(get_le(p, 8));
  h_.epochs_done = static_cast<int64_t>(get_le(p, 8));
  if (h_.n_feats <= 0 || h_.row_len < 0 || h_.row_len > (1ll << 32) || h_.n_changed < 0 || h_.n_changed > h_.n_feats || h_.chunk <= 0)
    throw std::runtime_error(path + ": sparse checkpoint header is inconsistent");
  r_ = std::make_unique<FloatFrameReader>(path, kSparseHeaderBytes);
  if (r_->total_floats() != body_words(h_))
    throw std::runtime_error(path + ": body length does not match the header (" + std::to_string(r_->total_floats()) +
                             " words, header implies " + std::to_string(body_words(h_)) + ")");
  ids_.resize(static_cast<size_t>(h_.n_changed));
  need(reinterpret_cast<float *>(ids_.data()), ids_.size());
  for (size_t j = 0; j < ids_.size(); j++)
    if (ids_[j] < 0 || ids_[j] >= h_.n_feats || (j > 0 && ids_[j] <= ids_[j - 1]))
      throw std::runtime_error(path + ": feature ids must ascend strictly inside [0, n_feats)");
}
SparseCheckpointReader::~SparseCheckpointReader() = default;
void SparseCheckpointReader::need(float *p, size_t n) {
  if (n && r_->read(p, n) != n) throw std::runtime_error(path_ + ": zstd frame is truncated");
}
size_t SparseCheckpointReader::next_chunk_size() const {
  return std::min(static_cast<size_t>(h_.n_changed) - done_, static_cast<size_t>(h_.chunk));
}
void SparseCheckpointReader::chunk(float *lin_w, float *lin_n, float *lin_z, float *vec_w, float *vec_n, float *vec_z) {
  const size_t c = next_chunk_size(), rl = static_cast<size_t>(h_.row_len);
  need(lin_w, c);
  need(lin_n, c);
  need(lin_z, c);
  if (rl) {
    need(vec_w, c * rl);
    need(vec_n, c * rl);
    need(vec_z, c * rl);
  }
  done_ += c;
}
void SparseCheckpointReader::finish() {
  if (next_chunk_size() != 0) throw std::logic_error("SparseCheckpointReader: records left unread");
  float extra;
  if (r_->read(&extra, 1) != 0) throw std::runtime_error(path_ + ": body is longer than the header implies");
}

// ffm.cpp:163-180: bias and lin_w through an ostream (default precision, 6 significant digits),
// latent rows as the shortest float representation that round-trips, space separated.
TextModelWriter::TextModelWriter(const std::string &path) : f_(path), path_(path) {
  if (!f_.good()) throw std::runtime_error("cannot write " + path);
}
void TextModelWriter::scalar(float v) { f_ << v << "\n"; }
void TextModelWriter::rows(const float *p, size_t n_rows, size_t row_len) {
  std::string out;
  out.reserve(n_rows * row_len * 12);
  char buf[64];
  for (size_t i = 0; i < n_rows; i++) {
    for (size_t j = 0; j < row_len; j++) {
      const int n = std::snprintf(buf, sizeof buf, "%.9g", static_cast<double>(p[i * row_len + j]));
      if (j) out.push_back(' ');
      out.append(buf, static_cast<size_t>(n));
    }
    out.push_back('\n');
  }
  f_ << out;
}
void TextModelWriter::finish() {
  f_.flush();
  if (!f_.good()) throw std::runtime_error("cannot write " + path_);
  f_.close();
}

// ffm.cpp:182-200
TextModelReader::TextModelReader(const std::string &path) : f_(path), path_(path) {
  if (!f_.good()) {
    std::fprintf(stderr, "Failed to open loading file %s\n", path.c_str());
    throw std::runtime_error("Failed to open loading file " + path);
  }
}
float TextModelReader::scalar() {
  std::getline(f_, line_);
  return std::stof(line_);
}
void TextModelReader::rows(float *p, size_t n_rows, size_t row_len) {
  for (size_t i = 0; i < n_rows; i++) {
    std::getline(f_, line_);
    const char *q = line_.c_str();
    for (size_t j = 0; j < row_len; j++) {
      char *end = nullptr;
      p[i * row_len + j] = std::strtof(q, &end);
      if (end == q) throw std::out_of_range("model file row too short: " + path_);
      q = end;
    }
  }
}

}  // namespace ftrl
