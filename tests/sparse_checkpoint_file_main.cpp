// Stand-alone check of the sparse checkpoint file format (ftrl-ffm_amd/host/persist.{h,cpp}): no engine,
// no device.  tests/test_sparse_checkpoint_file.py builds it with g++, plain and with
// -fsanitize=address,undefined, and runs it in a scratch directory given as argv[1].
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../ftrl-ffm_amd/host/persist.h"

using namespace ftrl;

static int g_failed = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failed++; } \
  } while (0)

static uint32_t word(uint64_t i) {  // any 32-bit pattern: NaNs, -0.0 and subnormals among them
  uint64_t x = (i + 1) * 0x9E3779B97F4A7C15ull;
  x ^= x >> 29;
  return static_cast<uint32_t>(x * 0xBF58476D1CE4E5B9ull >> 16);
}
static std::vector<float> words(size_t n, uint64_t salt) {
  std::vector<float> v(n);
  for (size_t i = 0; i < n; i++) {
    const uint32_t w = i == 0 ? 0x80000000u : i == 1 ? 0x7fc00001u : word(salt * 1000003ull + i);
    std::memcpy(&v[i], &w, 4);
  }
  return v;
}
static bool same_bits(const std::vector<float> &a, const std::vector<float> &b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * 4) == 0);
}

struct Model {
  SparseCheckpointHeader h;
  std::vector<int32_t> ids;
  std::vector<float> lin[3], vec[3];  // w, n, z of the changed features, in id order
};

static Model make(int model_type, int n_feats, int n_fields, int n_factors, int64_t row_len, int64_t n_changed,
                  int64_t chunk) {
  Model m;
  m.h.model_type = model_type;
  m.h.n_feats = n_feats;
  m.h.n_fields = n_fields;
  m.h.n_factors = n_factors;
  m.h.row_len = row_len;
  m.h.seed = 0xfedcba9876543210ull;
  m.h.init_mean_bits = 0x3e800000u;
  m.h.init_stddev_bits = 0x3ca3d70au;
  m.h.flags = 4;
  m.h.n_changed = n_changed;
  m.h.chunk = chunk;
  m.h.bias_bits[0] = 0xbf000000u;
  m.h.bias_bits[1] = 0x7fc00000u;
  m.h.bias_bits[2] = 0x80000000u;
  m.h.rows_seen = (1ll << 40) + 7;
  m.h.epochs_done = 3;
  for (int64_t j = 0; j < n_changed; j++)  // ascending, the first and the last id among them
    m.ids.push_back(static_cast<int32_t>(n_changed == 1 ? n_feats - 1 : j * (n_feats - 1) / (n_changed - 1)));
  for (int c = 0; c < 3; c++) {
    m.lin[c] = words(static_cast<size_t>(n_changed), 10 + c);
    m.vec[c] = words(static_cast<size_t>(n_changed * row_len), 20 + c);
  }
  return m;
}

static void write(const Model &m, const std::string &path) {
  SparseCheckpointWriter w(path, m.h, m.ids.data(), 3);
  const size_t rl = static_cast<size_t>(m.h.row_len), n = m.ids.size(), chunk = static_cast<size_t>(m.h.chunk);
  for (size_t j0 = 0; j0 < n; j0 += chunk) {
    const size_t c = std::min(chunk, n - j0);
    w.chunk(c, m.lin[0].data() + j0, m.lin[1].data() + j0, m.lin[2].data() + j0,
            rl ? m.vec[0].data() + j0 * rl : nullptr, rl ? m.vec[1].data() + j0 * rl : nullptr,
            rl ? m.vec[2].data() + j0 * rl : nullptr);
  }
  w.finish();
}

static Model read(const std::string &path) {
  SparseCheckpointReader r(path);
  Model m;
  m.h = r.header();
  m.ids = r.ids();
  const size_t rl = static_cast<size_t>(m.h.row_len), n = m.ids.size();
  for (int c = 0; c < 3; c++) { m.lin[c].resize(n); m.vec[c].resize(n * rl); }
  size_t j0 = 0;
  while (const size_t c = r.next_chunk_size()) {
    r.chunk(m.lin[0].data() + j0, m.lin[1].data() + j0, m.lin[2].data() + j0,
            rl ? m.vec[0].data() + j0 * rl : nullptr, rl ? m.vec[1].data() + j0 * rl : nullptr,
            rl ? m.vec[2].data() + j0 * rl : nullptr);
    j0 += c;
  }
  r.finish();
  return m;
}

static void round_trip(const char *name, const Model &m, const std::string &dir) {
  const std::string path = dir + "/" + name + ".ckpt";
  write(m, path);
  const Model g = read(path);
  CHECK(g.h.model_type == m.h.model_type && g.h.n_feats == m.h.n_feats && g.h.n_fields == m.h.n_fields &&
        g.h.n_factors == m.h.n_factors && g.h.row_len == m.h.row_len && g.h.flags == m.h.flags);
  CHECK(g.h.seed == m.h.seed && g.h.init_mean_bits == m.h.init_mean_bits && g.h.init_stddev_bits == m.h.init_stddev_bits);
  CHECK(g.h.n_changed == m.h.n_changed && g.h.chunk == m.h.chunk);
  CHECK(std::memcmp(g.h.bias_bits, m.h.bias_bits, sizeof m.h.bias_bits) == 0);
  CHECK(g.h.rows_seen == m.h.rows_seen && g.h.epochs_done == m.h.epochs_done);
  CHECK(g.ids == m.ids);
  for (int c = 0; c < 3; c++) CHECK(same_bits(g.lin[c], m.lin[c]) && same_bits(g.vec[c], m.vec[c]));
  std::printf("round trip %-16s n_changed=%lld row_len=%lld chunk=%lld ok\n", name, static_cast<long long>(m.h.n_changed),
              static_cast<long long>(m.h.row_len), static_cast<long long>(m.h.chunk));
}

static std::string slurp(const std::string &path) {
  std::ifstream f(path, std::ios::binary);
  return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
static void spit(const std::string &path, const std::string &bytes) {
  std::ofstream f(path, std::ios::binary);
  f.write(bytes.data(), static_cast<std::streamsize>(bytes.size()));
}

// the reader (header, ids, every chunk, end of frame) must throw std::runtime_error naming `expect`
static void rejects(const char *name, const std::string &path, const char *expect) {
  bool thrown = false;
  std::string msg;
  try {
    (void)read(path);
  } catch (const std::runtime_error &e) {
    thrown = true;
    msg = e.what();
  }
  if (!thrown || msg.find(expect) == std::string::npos) {
    std::printf("FAIL reject %s: %s\n", name, thrown ? msg.c_str() : "no std::runtime_error");
    g_failed++;
  } else {
    std::printf("reject %-24s ok (%s)\n", name, msg.c_str());
  }
}

int main(int argc, char **argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  if (!zstd_available()) {
    // persist's convention: without libzstd.so.1 the compressed formats throw std::runtime_error
    bool thrown = false;
    try {
      write(make(2, 10, 2, 2, 4, 1, 4), dir + "/nozstd.ckpt");
    } catch (const std::runtime_error &) {
      thrown = true;
    }
    CHECK(thrown);
    std::printf("libzstd absent: the writer throws std::runtime_error; %d failed\n", g_failed);
    return g_failed ? 1 : 0;
  }
  round_trip("ffm", make(2, 5000, 8, 4, 32, 137, 1000), dir);
  round_trip("fm", make(1, 777, 1, 16, 16, 300, 300), dir);
  round_trip("lr", make(0, 1000, 1, 0, 0, 1000, 64), dir);          // row_len = 0, every feature, 16 chunks
  round_trip("none_changed", make(2, 5000, 8, 4, 32, 0, 1000), dir);
  round_trip("one_changed", make(2, 5000, 8, 4, 32, 1, 1000), dir);
  round_trip("several_chunks", make(2, 100000, 8, 16, 128, 4099, 512), dir);  // 9 chunks, the last of 3 features
  round_trip("chunk_of_one", make(1, 64, 1, 3, 3, 5, 1), dir);

  const Model base = make(2, 5000, 8, 4, 32, 137, 50);
  const std::string good = dir + "/base.ckpt";
  write(base, good);
  const std::string bytes = slurp(good);
  CHECK(bytes.size() > kSparseHeaderBytes);
  {
    std::string b = bytes;
    b[0] = 'X';
    spit(dir + "/magic.ckpt", b);
    rejects("wrong magic", dir + "/magic.ckpt", "magic");
    spit(dir + "/dense.ckpt", bytes.substr(kSparseHeaderBytes));  // a bare zstd frame: the dense formats' file
    rejects("a dense model file", dir + "/dense.ckpt", "magic");
  }
  {
    std::string b = bytes;
    b[8] = 2;  // version
    spit(dir + "/version.ckpt", b);
    rejects("wrong version", dir + "/version.ckpt", "version");
  }
  {
    spit(dir + "/header_cut.ckpt", bytes.substr(0, 40));
    rejects("truncated header", dir + "/header_cut.ckpt", "truncated");
    spit(dir + "/frame_cut.ckpt", bytes.substr(0, bytes.size() - 9));
    rejects("truncated frame", dir + "/frame_cut.ckpt", "truncated");
    spit(dir + "/frame_cut_early.ckpt", bytes.substr(0, kSparseHeaderBytes + 30));
    rejects("truncated frame (early)", dir + "/frame_cut_early.ckpt", "truncated");
  }
  {
    // the header's n_changed no longer matches the body (offset 56: magic 8, version 4, five 32-bit
    // fields, row_len 8, seed 8, two 32-bit patterns)
    std::string b = bytes;
    b[56] = static_cast<char>(136);
    spit(dir + "/count.ckpt", b);
    rejects("n_changed != body", dir + "/count.ckpt", "body length");
    b = bytes;
    b[32] = 33;  // row_len
    spit(dir + "/row_len.ckpt", b);
    rejects("row_len != body", dir + "/row_len.ckpt", "body length");
  }
  {
    // ids that break the order / the range, framed correctly (what a foreign writer could produce)
    auto with_ids = [&](const char *name, std::function<void(Model &)> edit) {
      Model m = base;
      edit(m);
      SparseCheckpointHeader h = m.h;
      // the writer refuses such ids (std::invalid_argument): frame them by hand
      bool refused = false;
      try {
        SparseCheckpointWriter w(dir + "/refused.ckpt", h, m.ids.data(), 3);
      } catch (const std::invalid_argument &) {
        refused = true;
      }
      CHECK(refused);
      const size_t total = static_cast<size_t>(h.n_changed) * (4 + 3 * static_cast<size_t>(h.row_len));
      std::vector<float> body(total, 0.0f);
      std::memcpy(body.data(), m.ids.data(), m.ids.size() * 4);
      FloatFrameWriter w(dir + "/" + name + ".ckpt", total, 3, bytes.substr(0, kSparseHeaderBytes));
      w.write(body.data(), total);
      w.finish();
      rejects(name, dir + "/" + name + ".ckpt", "ascend");
    };
    with_ids("ids_equal", [](Model &m) { m.ids[5] = m.ids[4]; });
    with_ids("ids_descending", [](Model &m) { std::swap(m.ids[7], m.ids[8]); });
    with_ids("id_negative", [](Model &m) { m.ids[0] = -1; });
    with_ids("id_past_n_feats", [](Model &m) { m.ids.back() = m.h.n_feats; });
  }
  std::printf("%d failed\n", g_failed);
  return g_failed ? 1 : 0;
}
