// value_count.cpp -- --bucket_fields LIST: one pass over the training file before a model exists, as field_count.cpp
// and rare_count.cpp make theirs.  The parser's threads fill a block whose field and val arrays are page-locked, the
// device counts the (field, value bin) of its entries straight from there (the host does nothing per entry), and the
// host cuts each chosen field's 65536 counts into buckets of equal mass (ffm_engine_bucket_edges: exact integers).
#include <chrono>
#include <cstdio>
#include <stdexcept>

#include "count_block.h"
#include "text_stream.h"
#include "value_buckets.h"

namespace ftrl {

namespace {

void check_rc(int rc, const char *what) {
  if (rc != FFM_OK) throw std::runtime_error(std::string(what) + ": " + ffm_engine_last_error());
}

struct HistHandle {
  ffm_valhist *s = nullptr;
  ~HistHandle() { ffm_engine_valhist_destroy(s); }
};

}  // namespace

ValueBuckets count_value_buckets(const config_options &opt) {
  const auto t0 = std::chrono::steady_clock::now();
  const int F = opt.n_fields;
  HistHandle vh;
  {
    const int rc = ffm_engine_valhist_create(F, opt.device, &vh.s);
    if (rc == FFM_E_INVALID) throw std::invalid_argument(std::string("--bucket_fields: ") + ffm_engine_last_error());
    check_rc(rc, "ffm_engine_valhist_create");
  }
  unsigned long long rows = 0;
  if (opt.device_parse) {
    // --device_parse true: the file as raw bytes, parsed on the device into the arrays the histogram reads in HBM
    DeviceParseHooks hooks;
    hooks.device = [&](const ffm_text_block &b) {
      check_rc(ffm_engine_valhist_add_device(vh.s, static_cast<int32_t>(b.nnz), b.field, b.val), "ffm_engine_valhist_add_device");
    };
    hooks.host = [&](const CsrPart &p) {
      check_rc(ffm_engine_valhist_add(vh.s, static_cast<int32_t>(p.val.size()), p.field.data(), p.val.data(), 0), "ffm_engine_valhist_add");
    };
    hooks.sync = [&] { check_rc(ffm_engine_valhist_read(vh.s, nullptr, nullptr, nullptr, nullptr), "ffm_engine_valhist_read"); };
    rows = device_parse_pass(opt, hooks);
  } else {
    CountBlock cb(true);  // (no page-locked memory to be had: the histogram copies each block into its own)
    CsrStream stream(opt.train_path, opt.file_type, opt.thread_num);
    for (;;) {
      const size_t got = stream.next(kCountRows, cb.blk, kCountNnz, true);
      if (got == 0) break;
      rows += got;
      check_rc(ffm_engine_valhist_add(vh.s, static_cast<int32_t>(cb.blk.val.size()), cb.blk.field.data(), cb.blk.val.data(),
                                      cb.pinned ? 1 : 0),
               "ffm_engine_valhist_add");
    }
  }
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
