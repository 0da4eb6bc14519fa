// value_buckets.h -- --bucket_fields / --n_buckets / --buckets @FILE / --buckets_out (include/ffm_engine.h "Value
// buckets"): the bucket table every engine of a run maps numeric fields by, counted on the device from the training
// file or read from the file an earlier run wrote.  The table is not in checkpoints, exactly as the fields' ranges
// and the keep-map are not: a resumed, scoring or serving run passes --buckets @FILE.
//
// File: text.  One line `FFMBUCKETS <version> <n_fields>`, then one line `f k e1 .. ek` per bucketed field, fields
// ascending: the field, its number of edges (0 .. 255) and its edges (bins in [0, 65536), strictly ascending).
// value_buckets.cpp knows nothing of the engine; the counting pass and resolve_value_buckets are value_count.cpp.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "cmd_option.h"

namespace ftrl {

constexpr int kBucketMaxEdges = 255;  // FFM_BUCKET_MAX_EDGES
constexpr int kValueBucketsVersion = 1;

// A table as ffm_engine_set_buckets takes it: n_edges [n_fields] (-1: not bucketed), edges [n_fields][255].
struct ValueBuckets {
  int n_fields = 0;
  std::vector<int32_t> n_edges;
  std::vector<uint16_t> edges;
  explicit ValueBuckets(int fields = 0)
      : n_fields(fields), n_edges(static_cast<size_t>(fields), -1), edges(static_cast<size_t>(fields) * kBucketMaxEdges, 0) {}
};

// Throws std::invalid_argument when the table is not one, std::runtime_error when the file cannot be written.
void write_value_buckets(const std::string &path, const ValueBuckets &table);
// Reads and checks the whole file.  n_fields: the model's.  Throws std::invalid_argument, with the path in the
// message, on a file that cannot be opened, a wrong magic or version, another n_fields, a field outside
// [0, n_fields) or named twice or out of order, a count outside [0, 255], a missing or unreadable number, an edge
// outside [0, 65536), edges that do not ascend strictly, anything behind a line's last edge.
ValueBuckets read_value_buckets(const std::string &path, int n_fields);

// --bucket_fields: one pass over --train_data through a device histogram, the edge rule per chosen field, the lines
// `field f: N values in D bins -> K buckets` and `value buckets: counted ...`.  (value_count.cpp; needs a device.)
ValueBuckets count_value_buckets(const config_options &opt);
// What main.cpp calls before resolve_rare_ids: fills opt.bucket_n_edges / opt.bucket_edges from --bucket_fields or
// --buckets @FILE and writes --buckets_out.  Nothing asked for: nothing done.
void resolve_value_buckets(config_options &opt);

}  // namespace ftrl
