// value_count.cpp -- --bucket_fields LIST: one pass over the training file before a model exists (count_pass.h).  The
// device counts the (field, value bin) of the entries, and the host cuts each chosen field's 65536 counts into
// buckets of equal mass (ffm_engine_bucket_edges: exact integers).
#include <chrono>
#include <cstdio>
#include <stdexcept>

#include "count_pass.h"
#include "value_buckets.h"

namespace ftrl {

ValueBuckets count_value_buckets(const config_options &opt) {
  const auto t0 = std::chrono::steady_clock::now();
  const int F = opt.n_fields;
  CountHandle<ffm_valhist, ffm_engine_valhist_destroy> vh;
  {
    const int rc = ffm_engine_valhist_create(F, opt.device, &vh.s);
    if (rc == FFM_E_INVALID) throw std::invalid_argument(std::string("--bucket_fields: ") + ffm_engine_last_error());
    check_rc(rc, "ffm_engine_valhist_create");
  }
  CountPass pass;
  pass.with_val = true;
  pass.add_device = [&](int32_t nnz, const int32_t *field, const int32_t *, const float *val) {
    check_rc(ffm_engine_valhist_add_device(vh.s, nnz, field, val), "ffm_engine_valhist_add_device");
  };
  pass.add = [&](int32_t nnz, const int32_t *field, const int32_t *, const float *val, int zero_copy) {
    check_rc(ffm_engine_valhist_add(vh.s, nnz, field, val, zero_copy), "ffm_engine_valhist_add");
  };
  pass.sync = [&] { check_rc(ffm_engine_valhist_read(vh.s, nullptr, nullptr, nullptr, nullptr), "ffm_engine_valhist_read"); };
  const unsigned long long rows = count_pass(opt, pass);
  std::vector<uint64_t> counts(static_cast<size_t>(F) * FFM_BUCKET_BINS);
  int64_t n_valid = 0, n_bad = 0, n_nan = 0;
  check_rc(ffm_engine_valhist_read(vh.s, counts.data(), &n_valid, &n_bad, &n_nan), "ffm_engine_valhist_read");
  ValueBuckets table(F);
  for (int f : opt.bucket_field_list) {
    const uint64_t *c = counts.data() + static_cast<size_t>(f) * FFM_BUCKET_BINS;
    unsigned long long n = 0, bins = 0;
    for (int b = 0; b < FFM_BUCKET_BINS; b++) {
      n += c[b];
      bins += c[b] != 0;
    }
    int32_t k = 0;
    check_rc(ffm_engine_bucket_edges(c, opt.n_buckets, table.edges.data() + static_cast<size_t>(f) * kBucketMaxEdges, &k),
             "ffm_engine_bucket_edges");
    table.n_edges[static_cast<size_t>(f)] = k;
    std::printf("field %d: %llu values in %llu bins -> %d buckets\n", f, n, bins, k + 1);
  }
  std::printf("value buckets: counted %llu rows (%lld entries, %lld nan) in %.4lf s\n", rows, static_cast<long long>(n_valid + n_bad),
              static_cast<long long>(n_nan), std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  return table;
}

void resolve_value_buckets(config_options &opt) {
  ValueBuckets table;
  if (!opt.bucket_fields.empty()) table = count_value_buckets(opt);
  else if (!opt.buckets.empty()) table = read_value_buckets(opt.buckets.substr(1), opt.n_fields);
  else return;
  if (!opt.buckets_out.empty()) write_value_buckets(opt.buckets_out, table);
  opt.bucket_n_edges = std::move(table.n_edges);
  opt.bucket_edges = std::move(table.edges);
}

}  // namespace ftrl
