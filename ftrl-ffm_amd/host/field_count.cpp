// field_count.cpp -- --field_ranges counted: one pass over the training file before a model exists (count_pass.h).
// The device counts the (field, feat) entries into a sketch, and the estimates size the fields' id ranges.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <stdexcept>

#include "count_pass.h"
#include "field_ranges.h"

namespace ftrl {

std::vector<int32_t> count_field_ranges(const config_options &opt) {
  const auto t0 = std::chrono::steady_clock::now();
  const int F = opt.n_fields;
  CountHandle<ffm_sketch, ffm_engine_sketch_destroy> sk;
  {
    const int rc = ffm_engine_sketch_create(F, opt.device, &sk.s);
    if (rc == FFM_E_INVALID) throw std::invalid_argument(ffm_engine_last_error());
    check_rc(rc, "ffm_engine_sketch_create");
  }
  // --min_count / --rare_ids: the ranges are sized by the ids that stay -- a rare id counts as its field's one rare id
  if (!opt.rare_words.empty())
    check_rc(ffm_engine_sketch_set_filter(sk.s, opt.rare_map_bits, opt.rare_words.data()), "ffm_engine_sketch_set_filter");
  CountPass pass;
  pass.add_device = [&](int32_t nnz, const int32_t *field, const int32_t *feat, const float *) {
    check_rc(ffm_engine_sketch_add_device(sk.s, nnz, field, feat), "ffm_engine_sketch_add_device");
  };
  pass.add = [&](int32_t nnz, const int32_t *field, const int32_t *feat, const float *, int zero_copy) {
    check_rc(ffm_engine_sketch_add(sk.s, nnz, field, feat, zero_copy), "ffm_engine_sketch_add");
  };
  pass.sync = [&] { check_rc(ffm_engine_sketch_read(sk.s, nullptr, nullptr, nullptr), "ffm_engine_sketch_read"); };
  const unsigned long long rows = count_pass(opt, pass);
  std::vector<uint8_t> reg(static_cast<size_t>(F) * FFM_SKETCH_REGS);
  int64_t n_valid = 0, n_bad = 0;
  check_rc(ffm_engine_sketch_read(sk.s, reg.data(), &n_valid, &n_bad), "ffm_engine_sketch_read");
  std::vector<double> est(static_cast<size_t>(F));
  check_rc(ffm_engine_sketch_estimate(reg.data(), F, est.data()), "ffm_engine_sketch_estimate");
  std::vector<int64_t> count(static_cast<size_t>(F));
  long long total = 0;
  for (int f = 0; f < F; f++) {
    count[f] = std::max<long long>(1, std::llround(est[f]));
    // --bucket_fields / --buckets: a bucketed field's ids are its buckets and the NaN id, whatever its one raw id
    if (!opt.bucket_n_edges.empty() && opt.bucket_n_edges[static_cast<size_t>(f)] >= 0) count[f] = opt.bucket_n_edges[static_cast<size_t>(f)] + 2;
    total += count[f];
  }
  std::vector<int32_t> fs(static_cast<size_t>(F) + 1);
  {
    const int rc = ffm_engine_field_ranges(count.data(), F, opt.n_feats, fs.data());
    if (rc == FFM_E_INVALID) throw std::invalid_argument(std::string("--field_ranges counted: ") + ffm_engine_last_error());
    check_rc(rc, "ffm_engine_field_ranges");
  }
  for (int f = 0; f < F; f++)
    std::printf("field %d: ~%lld distinct ids, ids [%d, %d)\n", f, static_cast<long long>(count[f]), fs[f], fs[f + 1]);
  std::printf("field ranges: counted from %llu rows (%lld entries, %lld erased) in %.4lf s; ~%lld distinct ids for %d features (load %.3lf)\n",
              rows, static_cast<long long>(n_valid + n_bad), static_cast<long long>(n_bad),
              std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), total, opt.n_feats,
              static_cast<double>(total) / static_cast<double>(opt.n_feats));
  return fs;
}

void resolve_field_ranges(config_options &opt) {
  if (opt.field_ranges == "counted") opt.field_start = count_field_ranges(opt);
  else if (!opt.field_ranges.empty() && opt.field_ranges[0] == '@')
    opt.field_start = read_field_ranges(opt.field_ranges.substr(1), opt.n_fields, opt.n_feats, opt.hash_feats);
  if (opt.field_ranges_out.empty()) return;
  write_field_ranges(opt.field_ranges_out,
                     opt.field_start.empty() ? uniform_field_ranges(opt.n_fields, opt.n_feats) : opt.field_start);
}

}  // namespace ftrl
