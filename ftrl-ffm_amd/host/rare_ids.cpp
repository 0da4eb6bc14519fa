// rare_ids.cpp -- the keep-map file (rare_ids.h): a fixed little-endian header and one zstd frame.
#include "rare_ids.h"

#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "persist.h"

namespace ftrl {

namespace {
const char kRareMagic[8] = {'F', 'F', 'M', 'R', 'A', 'R', 'E', '\n'};

void put_le(std::string &out, uint64_t v, int bytes) {
  for (int i = 0; i < bytes; i++) out.push_back(static_cast<char>((v >> (8 * i)) & 0xff));
}
uint64_t get_le(const unsigned char *&p, int bytes) {
  uint64_t v = 0;
  for (int i = 0; i < bytes; i++) v |= static_cast<uint64_t>(p[i]) << (8 * i);
  p += bytes;
  return v;
}
size_t words_of(int bits) { return (static_cast<size_t>(1) << bits) / 64; }
uint64_t popcount(const std::vector<uint64_t> &words) {
  uint64_t n = 0;
  for (uint64_t w : words) n += static_cast<uint64_t>(__builtin_popcountll(w));
  return n;
}
}  // namespace

int default_rare_bits(int n_feats) {
  int bits = 16;
  while (bits < 30 && (1ll << bits) < 4ll * n_feats) bits++;
  return bits;
}

uint64_t rare_ids_checksum(const std::vector<uint64_t> &words) {
  uint64_t h = 14695981039346656037ull;
  for (uint64_t w : words) h = (h ^ w) * 1099511628211ull;
  return h;
}

void write_rare_ids(const std::string &path, const RareIds &map) {
  if (map.bits < 8 || map.bits > 30 || map.words.size() != words_of(map.bits) || map.n_fields < 0 || map.min_count < 1)
    throw std::invalid_argument("write_rare_ids: not a keep-map");
  std::string head(kRareMagic, sizeof kRareMagic);
  put_le(head, kRareIdsVersion, 4);
  put_le(head, static_cast<uint32_t>(map.bits), 4);
  put_le(head, static_cast<uint32_t>(map.min_count), 4);
  put_le(head, static_cast<uint32_t>(map.n_fields), 4);
  put_le(head, map.rows, 8);
  put_le(head, popcount(map.words), 8);
  put_le(head, rare_ids_checksum(map.words), 8);
  if (head.size() != kRareIdsHeaderBytes) throw std::logic_error("write_rare_ids: header size");
  // the words as 32-bit halves, low half first, whatever the host's byte order
  std::vector<uint32_t> halves(2 * map.words.size());
  for (size_t i = 0; i < map.words.size(); i++) {
    halves[2 * i] = static_cast<uint32_t>(map.words[i]);
    halves[2 * i + 1] = static_cast<uint32_t>(map.words[i] >> 32);
  }
  std::vector<float> body(halves.size());
  std::memcpy(body.data(), halves.data(), halves.size() * sizeof(uint32_t));
  FloatFrameWriter w(path, body.size(), 3, head);
  w.write(body.data(), body.size());
  w.finish();
}

RareIds read_rare_ids(const std::string &path, int n_fields, int bits) {
  auto bad = [&](const std::string &msg) { return std::invalid_argument(path + ": " + msg); };
  unsigned char raw[kRareIdsHeaderBytes];
  {
    std::FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) throw bad("cannot be opened");
    const size_t got = std::fread(raw, 1, sizeof raw, f);
    std::fclose(f);
    if (got < sizeof kRareMagic || std::memcmp(raw, kRareMagic, sizeof kRareMagic) != 0)
      throw bad("not a keep-map of rare ids (wrong magic)");
    if (got != sizeof raw) throw bad("the keep-map's header is truncated");
  }
  const unsigned char *p = raw + sizeof kRareMagic;
  const uint32_t version = static_cast<uint32_t>(get_le(p, 4));
  if (version != kRareIdsVersion)
    throw bad("keep-map version " + std::to_string(version) + ", this build reads " + std::to_string(kRareIdsVersion));
  RareIds map;
  const uint32_t file_bits = static_cast<uint32_t>(get_le(p, 4)), min_count = static_cast<uint32_t>(get_le(p, 4));
  const uint32_t file_fields = static_cast<uint32_t>(get_le(p, 4));
  map.rows = get_le(p, 8);
  map.kept_slots = get_le(p, 8);
  const uint64_t checksum = get_le(p, 8);
  if (file_bits < 8 || file_bits > 30 || min_count < 1 || min_count > 65535 || file_fields > 0x7fffffffu)
    throw bad("the keep-map's header is inconsistent");
  map.bits = static_cast<int>(file_bits);
  map.min_count = static_cast<int>(min_count);
  map.n_fields = static_cast<int>(file_fields);
  if (map.n_fields != n_fields)
    throw bad("was counted for " + (map.n_fields ? std::to_string(map.n_fields) + " fields" : std::string("a model without fields")) +
              ", this model has " + (n_fields ? std::to_string(n_fields) + " fields" : std::string("none")));
  if (bits != 0 && bits != map.bits)
    throw bad("holds 2^" + std::to_string(map.bits) + " slots, --rare_bits asks for 2^" + std::to_string(bits));
  try {
    FloatFrameReader r(path, kRareIdsHeaderBytes);
    if (r.total_floats() != 2 * words_of(map.bits))
      throw bad("the frame holds " + std::to_string(r.total_floats() / 2) + " words, the header's bits = " +
                std::to_string(map.bits) + " imply " + std::to_string(words_of(map.bits)));
    std::vector<float> body(2 * words_of(map.bits));
    if (r.read(body.data(), body.size()) != body.size()) throw bad("zstd frame is truncated");
    float extra;
    if (r.read(&extra, 1) != 0) throw bad("the frame is longer than the header implies");
    std::vector<uint32_t> halves(body.size());
    std::memcpy(halves.data(), body.data(), body.size() * sizeof(uint32_t));
    map.words.resize(words_of(map.bits));
    for (size_t i = 0; i < map.words.size(); i++) map.words[i] = halves[2 * i] | static_cast<uint64_t>(halves[2 * i + 1]) << 32;
  } catch (const std::invalid_argument &) {
    throw;
  } catch (const std::runtime_error &e) {  // (the frame reader's: truncated, corrupt, not zstd -- the path is in its message)
    throw std::invalid_argument(e.what());
  }
  if (rare_ids_checksum(map.words) != checksum) throw bad("the words do not have the header's checksum: the keep-map is damaged");
  if (popcount(map.words) != map.kept_slots) throw bad("the words do not have the header's number of kept slots");
  return map;
}

}  // namespace ftrl
