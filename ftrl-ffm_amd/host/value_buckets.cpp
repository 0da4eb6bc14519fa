// value_buckets.cpp -- the bucket table file (value_buckets.h): a header line and one line per bucketed field.
#include "value_buckets.h"

#include <fstream>
#include <sstream>
#include <stdexcept>

namespace ftrl {

namespace {
const char kBucketsMagic[] = "FFMBUCKETS";

bool table_ok(const ValueBuckets &t) {
  if (t.n_fields <= 0 || t.n_edges.size() != static_cast<size_t>(t.n_fields) ||
      t.edges.size() != static_cast<size_t>(t.n_fields) * kBucketMaxEdges)
    return false;
  for (int f = 0; f < t.n_fields; f++) {
    const int k = t.n_edges[static_cast<size_t>(f)];
    if (k < -1 || k > kBucketMaxEdges) return false;
    const uint16_t *e = t.edges.data() + static_cast<size_t>(f) * kBucketMaxEdges;
    for (int i = 1; i < k; i++)
      if (e[i] <= e[i - 1]) return false;
  }
  return true;
}
}  // namespace

void write_value_buckets(const std::string &path, const ValueBuckets &t) {
  if (!table_ok(t)) throw std::invalid_argument("write_value_buckets: not a bucket table");
  std::ofstream out(path, std::ios::trunc);
  out << kBucketsMagic << ' ' << kValueBucketsVersion << ' ' << t.n_fields << '\n';
  for (int f = 0; f < t.n_fields; f++) {
    const int k = t.n_edges[static_cast<size_t>(f)];
    if (k < 0) continue;
    out << f << ' ' << k;
    for (int i = 0; i < k; i++) out << ' ' << t.edges[static_cast<size_t>(f) * kBucketMaxEdges + static_cast<size_t>(i)];
    out << '\n';
  }
  out.flush();
  if (!out.good()) throw std::runtime_error(path + ": the bucket table cannot be written");
}

ValueBuckets read_value_buckets(const std::string &path, int n_fields) {
  auto bad = [&](const std::string &msg) { return std::invalid_argument(path + ": " + msg); };
  std::ifstream in(path);
  if (!in.good()) throw bad("cannot be opened");
  std::string line;
  if (!std::getline(in, line)) throw bad("not a bucket table (empty file)");
  {
    std::istringstream is(line);
    std::string magic, extra;
    long long version = -1, fields = -1;
    is >> magic;
    if (magic != kBucketsMagic) throw bad("not a bucket table (wrong magic)");
    if (!(is >> version >> fields) || (is >> extra)) throw bad("the bucket table's header is damaged");
    if (version != kValueBucketsVersion)
      throw bad("bucket table version " + std::to_string(version) + ", this build reads " + std::to_string(kValueBucketsVersion));
    if (fields != n_fields)
      throw bad("was counted for " + std::to_string(fields) + " fields, this model has " + std::to_string(n_fields));
  }
  ValueBuckets t(n_fields);
  long long last_field = -1;
  size_t line_no = 1;
  while (std::getline(in, line)) {
    line_no++;
    if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
    const std::string where = "line " + std::to_string(line_no) + ": ";
    std::istringstream is(line);
    long long f = -1, k = -1;
    if (!(is >> f >> k)) throw bad(where + "expected `field count edges..`");
    if (f < 0 || f >= n_fields) throw bad(where + "field " + std::to_string(f) + " is outside [0, " + std::to_string(n_fields) + ")");
    if (f <= last_field) throw bad(where + "field " + std::to_string(f) + " is named twice or out of order");
    last_field = f;
    if (k < 0 || k > kBucketMaxEdges) throw bad(where + "a field has 0 .. 255 edges, got " + std::to_string(k));
    long long prev = -1;
    for (long long i = 0; i < k; i++) {
      long long e = -1;
      if (!(is >> e)) throw bad(where + "holds fewer than its " + std::to_string(k) + " edges");
      if (e < 0 || e > 65535) throw bad(where + "edge " + std::to_string(e) + " is outside [0, 65536)");
      if (e <= prev) throw bad(where + "the edges must be strictly ascending");
      prev = e;
      t.edges[static_cast<size_t>(f) * kBucketMaxEdges + static_cast<size_t>(i)] = static_cast<uint16_t>(e);
    }
    std::string extra;
    if (is >> extra) throw bad(where + "holds more than its " + std::to_string(k) + " edges");
    t.n_edges[static_cast<size_t>(f)] = static_cast<int32_t>(k);
  }
  return t;
}

}  // namespace ftrl
