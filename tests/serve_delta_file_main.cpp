// Stand-alone check of the serving delta file format (ftrl-ffm_amd/host/serve_delta.{h,cpp}): no engine, no
// device.  tests/test_serve_delta_file.py builds it with g++ from persist.cpp and serve_delta.cpp, plain and with
// -fsanitize=address,undefined, and runs it in a scratch directory given as argv[1].
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../ftrl-ffm_amd/host/serve_delta.h"

using namespace ftrl;

static int g_failed = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failed++; } \
  } while (0)

static uint32_t word(uint64_t i) {  // any 32-bit pattern: NaNs with payloads, -0.0 and subnormals among them
  uint64_t x = (i + 1) * 0x9E3779B97F4A7C15ull;
  x ^= x >> 29;
  return static_cast<uint32_t>(x * 0xBF58476D1CE4E5B9ull >> 16);
}

struct Delta {
  ServeDeltaHeader h;
  std::vector<int32_t> ids;
  std::vector<uint32_t> lin;   // lin_w patterns of the moved features, in id order
  std::vector<uint16_t> lat16; // the rows' bits (f16) ...
  std::vector<uint32_t> lat32; // ... or (f32)
  const void *lat_at(size_t j) const {
    const size_t rl = static_cast<size_t>(h.row_len);
    return h.format == kServeDeltaF16 ? static_cast<const void *>(lat16.data() + j * rl) : static_cast<const void *>(lat32.data() + j * rl);
  }
  void *lat_at(size_t j) { return const_cast<void *>(static_cast<const Delta *>(this)->lat_at(j)); }
};

static Delta make(uint32_t format, int n_feats, int n_fields, int n_factors, int64_t n_moved, int64_t chunk, int64_t seq) {
  Delta d;
  d.h.model_type = 2;
  d.h.n_feats = n_feats;
  d.h.n_fields = n_fields;
  d.h.n_factors = n_factors;
  d.h.hash_ids = static_cast<uint32_t>(seq & 1);
  d.h.format = format;
  d.h.row_len = static_cast<int64_t>(n_fields) * n_factors;
  d.h.seed = 0xfedcba9876543210ull;
  d.h.init_mean_bits = 0x3e800000u;
  d.h.init_stddev_bits = 0x3ca3d70au;
  d.h.seq = seq;
  d.h.n_moved = n_moved;
  d.h.chunk = chunk;
  d.h.bias_bits = 0x7fc00123u;
  for (int64_t j = 0; j < n_moved; j++)  // ascending, the first and the last id among them
    d.ids.push_back(static_cast<int32_t>(n_moved == 1 ? n_feats - 1 : j * (n_feats - 1) / (n_moved - 1)));
  const size_t n = static_cast<size_t>(n_moved), rl = static_cast<size_t>(d.h.row_len);
  for (size_t j = 0; j < n; j++) d.lin.push_back(j == 0 ? 0x80000000u : j == 1 ? 0x7fc00001u : word(7000003ull + j));
  if (format == kServeDeltaF16)
    for (size_t e = 0; e < n * rl; e++) d.lat16.push_back(e == 0 ? 0x8000 : e == 1 ? 0x7e55 : static_cast<uint16_t>(word(e)));
  else
    for (size_t e = 0; e < n * rl; e++) d.lat32.push_back(e == 0 ? 0x80000000u : e == 1 ? 0x7fc12345u : word(e));
  return d;
}

static void write(const Delta &d, const std::string &path) {
  ServeDeltaWriter w(path, d.h, d.ids.data(), 3);
  const size_t n = d.ids.size(), chunk = static_cast<size_t>(d.h.chunk);
  for (size_t j0 = 0; j0 < n; j0 += chunk) {
    const size_t c = std::min(chunk, n - j0);
    w.chunk(c, reinterpret_cast<const float *>(d.lin.data() + j0), d.lat_at(j0));
  }
  w.finish();
}

static Delta read(const std::string &path) {
  ServeDeltaReader r(path);
  Delta d;
  d.h = r.header();
  d.ids = r.ids();
  const size_t n = d.ids.size(), rl = static_cast<size_t>(d.h.row_len);
  d.lin.resize(n);
  if (d.h.format == kServeDeltaF16) d.lat16.resize(n * rl); else d.lat32.resize(n * rl);
  size_t j0 = 0;
  while (const size_t c = r.next_chunk_size()) {
    r.chunk(reinterpret_cast<float *>(d.lin.data() + j0), d.lat_at(j0));
    j0 += c;
  }
  r.finish();
  return d;
}

static void round_trip(const std::string &name, const Delta &d, const std::string &dir) {
  const std::string path = dir + "/" + name + ".delta";
  write(d, path);
  CHECK(read_serve_delta_header(path).seq == d.h.seq);
  const Delta g = read(path);
  CHECK(g.h.model_type == d.h.model_type && g.h.n_feats == d.h.n_feats && g.h.n_fields == d.h.n_fields &&
        g.h.n_factors == d.h.n_factors && g.h.row_len == d.h.row_len && g.h.hash_ids == d.h.hash_ids && g.h.format == d.h.format);
  CHECK(g.h.seed == d.h.seed && g.h.init_mean_bits == d.h.init_mean_bits && g.h.init_stddev_bits == d.h.init_stddev_bits);
  CHECK(g.h.seq == d.h.seq && g.h.n_moved == d.h.n_moved && g.h.chunk == d.h.chunk && g.h.bias_bits == d.h.bias_bits);
  CHECK(g.ids == d.ids && g.lin == d.lin && g.lat16 == d.lat16 && g.lat32 == d.lat32);
  std::printf("round trip %-20s format=%u n_moved=%lld row_len=%lld chunk=%lld ok\n", name.c_str(), d.h.format,
              static_cast<long long>(d.h.n_moved), static_cast<long long>(d.h.row_len), static_cast<long long>(d.h.chunk));
}

static std::string slurp(const std::string &path) {
  std::ifstream f(path, std::ios::binary);
  return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
static void spit(const std::string &path, const std::string &bytes) {
  std::ofstream f(path, std::ios::binary);
  f.write(bytes.data(), static_cast<std::streamsize>(bytes.size()));
}

// the reader (header, ids, every chunk, end of frame) must throw std::runtime_error naming `expect` and the path
static void rejects(const char *name, const std::string &path, const char *expect) {
  bool thrown = false;
  std::string msg;
  try {
    (void)read(path);
  } catch (const std::runtime_error &e) {
    thrown = true;
    msg = e.what();
  }
  if (!thrown || msg.find(expect) == std::string::npos || msg.find(path) == std::string::npos) {
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
      write(make(kServeDeltaF32, 10, 2, 4, 1, 4, 1), dir + "/nozstd.delta");
    } catch (const std::runtime_error &) {
      thrown = true;
    }
    CHECK(thrown);
    std::printf("libzstd absent: the writer throws std::runtime_error; %d failed\n", g_failed);
    return g_failed ? 1 : 0;
  }
  const int64_t chunk = 64;
  for (uint32_t format : {kServeDeltaF32, kServeDeltaF16})
    for (int64_t n_moved : {int64_t(0), int64_t(1), chunk, chunk + 1})
      round_trip(std::string(format == kServeDeltaF16 ? "f16_" : "f32_") + std::to_string(n_moved),
                 make(format, 5000, 5, 4, n_moved, chunk, 1 + n_moved), dir);

  for (uint32_t format : {kServeDeltaF32, kServeDeltaF16}) {
    const std::string tag = format == kServeDeltaF16 ? "f16" : "f32";
    const Delta base = make(format, 5000, 8, 4, 137, 50, 3);
    const std::string good = dir + "/base_" + tag + ".delta";
    write(base, good);
    const std::string bytes = slurp(good);
    CHECK(bytes.size() > kServeDeltaHeaderBytes);
    auto at = [&](const char *name) { return dir + "/" + name + "_" + tag + ".delta"; };
    {
      std::string b = bytes;
      b[0] = 'X';
      spit(at("magic"), b);
      rejects("wrong magic", at("magic"), "magic");
      spit(at("bare"), bytes.substr(kServeDeltaHeaderBytes));  // a bare zstd frame: a dense model file
      rejects("a dense model file", at("bare"), "magic");
      b = bytes;
      b[8] = 2;  // version
      spit(at("version"), b);
      rejects("wrong version", at("version"), "version");
    }
    {
      spit(at("header_cut"), bytes.substr(0, 40));
      rejects("truncated header", at("header_cut"), "truncated");
      spit(at("frame_cut"), bytes.substr(0, bytes.size() - 9));
      rejects("truncated frame", at("frame_cut"), "truncated");
      spit(at("frame_cut_early"), bytes.substr(0, kServeDeltaHeaderBytes + 30));
      rejects("truncated frame (early)", at("frame_cut_early"), "truncated");
    }
    {
      // the header no longer matches the body: n_moved at offset 72, row_len at 40 (magic 8, version 4, six
      // 32-bit fields and 4 bytes of padding; row_len 8, seed 8, two 32-bit patterns, seq 8)
      std::string b = bytes;
      b[72] = static_cast<char>(136);
      spit(at("count"), b);
      rejects("n_moved != body", at("count"), "body length");
      b = bytes;
      b[40] = 36;  // row_len
      spit(at("row_len"), b);
      rejects("row_len != body", at("row_len"), "body length");
    }
    {
      // ids that break the order / the range, framed correctly (what a foreign writer could produce)
      auto with_ids = [&](const char *name, std::function<void(Delta &)> edit) {
        Delta d = base;
        edit(d);
        bool refused = false;  // the writer refuses such ids (std::invalid_argument): frame them by hand
        try {
          ServeDeltaWriter w(dir + "/refused.delta", d.h, d.ids.data(), 3);
        } catch (const std::invalid_argument &) {
          refused = true;
        }
        CHECK(refused);
        const size_t total = d.h.body_words();
        std::vector<float> body(total, 0.0f);
        std::memcpy(body.data(), d.ids.data(), d.ids.size() * 4);
        FloatFrameWriter w(at(name), total, 3, bytes.substr(0, kServeDeltaHeaderBytes));
        w.write(body.data(), total);
        w.finish();
        rejects(name, at(name), "ascend");
      };
      with_ids("ids_equal", [](Delta &d) { d.ids[5] = d.ids[4]; });
      with_ids("ids_descending", [](Delta &d) { std::swap(d.ids[7], d.ids[8]); });
      with_ids("id_negative", [](Delta &d) { d.ids[0] = -1; });
      with_ids("id_past_n_feats", [](Delta &d) { d.ids.back() = d.h.n_feats; });
    }
  }
  std::printf("%d failed\n", g_failed);
  return g_failed ? 1 : 0;
}
