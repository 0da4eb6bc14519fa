// field_count.cpp -- --field_ranges counted: one pass over the training file before a model exists.  The
// parser's threads fill a page-locked block, the device counts its (field, feat) entries into a sketch
// straight from there (the host does nothing per entry), and the estimates size the fields' id ranges.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <stdexcept>

#include "count_block.h"
#include "field_ranges.h"
#include "text_stream.h"

namespace ftrl {

namespace {

void check_rc(int rc, const char *what) {
  if (rc != FFM_OK) throw std::runtime_error(std::string(what) + ": " + ffm_engine_last_error());
}

struct SketchHandle {
  ffm_sketch *s = nullptr;
  ~SketchHandle() { ffm_engine_sketch_destroy(s); }
};

}  // namespace

std::vector<int32_t> count_field_ranges(const config_options &opt) {
  const auto t0 = std::chrono::steady_clock::now();
  const int F = opt.n_fields;
  SketchHandle sk;
  {
    const int rc = ffm_engine_sketch_create(F, opt.device, &sk.s);
    if (rc == FFM_E_INVALID) throw std::invalid_argument(ffm_engine_last_error());
    check_rc(rc, "ffm_engine_sketch_create");
  }
  // --min_count / --rare_ids: the ranges are sized by the ids that stay -- a rare id counts as its field's one rare id
  if (!opt.rare_words.empty())
    check_rc(ffm_engine_sketch_set_filter(sk.s, opt.rare_map_bits, opt.rare_words.data()), "ffm_engine_sketch_set_filter");
  unsigned long long rows = 0;
  if (opt.device_parse) {
    // --device_parse true: the file as raw bytes, parsed on the device into the arrays the sketch reads in HBM
    DeviceParseHooks hooks;
    hooks.device = [&](const ffm_text_block &b) {
      check_rc(ffm_engine_sketch_add_device(sk.s, static_cast<int32_t>(b.nnz), b.field, b.feat), "ffm_engine_sketch_add_device");
    };
    hooks.host = [&](const CsrPart &p) {
      check_rc(ffm_engine_sketch_add(sk.s, static_cast<int32_t>(p.feat.size()), p.field.data(), p.feat.data(), 0), "ffm_engine_sketch_add");
    };
    hooks.sync = [&] { check_rc(ffm_engine_sketch_read(sk.s, nullptr, nullptr, nullptr), "ffm_engine_sketch_read"); };
    rows = device_parse_pass(opt, hooks);
  } else {
    CountBlock cb;  // (no page-locked memory to be had: the sketch copies each block into its own)
    CsrStream stream(opt.train_path, opt.file_type, opt.thread_num);
    for (;;) {
      const size_t got = stream.next(kCountRows, cb.blk, kCountNnz, true);
      if (got == 0) break;
      rows += got;
      check_rc(ffm_engine_sketch_add(sk.s, static_cast<int32_t>(cb.blk.feat.size()), cb.blk.field.data(), cb.blk.feat.data(),
                                     cb.pinned ? 1 : 0),
               "ffm_engine_sketch_add");
    }
  }
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
