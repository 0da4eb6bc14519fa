// rare_count.cpp -- --min_count T: one pass over the training file before a model exists, as field_count.cpp makes
// one for the cardinalities.  The parser's threads fill a page-locked block, the device counts the hashed slot of
// its (field, feat) entries straight from there (the host does nothing per entry), one small kernel turns the counts
// into the keep-map.  With --field_ranges counted the file is then streamed once more through a FILTERED sketch
// (count_field_ranges), so that the ranges are sized by the ids that stay.
#include <chrono>
#include <cstdio>
#include <stdexcept>

#include "count_block.h"
#include "rare_ids.h"
#include "text_stream.h"

namespace ftrl {

namespace {

void check_rc(int rc, const char *what) {
  if (rc != FFM_OK) throw std::runtime_error(std::string(what) + ": " + ffm_engine_last_error());
}

struct CounterHandle {
  ffm_idcount *s = nullptr;
  ~CounterHandle() { ffm_engine_idcount_destroy(s); }
};

int model_fields(const config_options &opt) { return opt.model_type == "FFM" ? opt.n_fields : 0; }

}  // namespace

RareIds count_rare_ids(const config_options &opt) {
  const auto t0 = std::chrono::steady_clock::now();
  RareIds map;
  map.bits = opt.rare_bits ? opt.rare_bits : default_rare_bits(opt.n_feats);
  map.min_count = opt.min_count;
  map.n_fields = model_fields(opt);
  CounterHandle ct;
  {
    const int rc = ffm_engine_idcount_create(map.n_fields, map.bits, map.min_count, opt.device, &ct.s);
    if (rc == FFM_E_INVALID) throw std::invalid_argument(std::string("--min_count: ") + ffm_engine_last_error());
    check_rc(rc, "ffm_engine_idcount_create");
  }
  if (opt.device_parse) {
    // --device_parse true: the file as raw bytes, parsed on the device into the arrays the counter reads in HBM
    DeviceParseHooks hooks;
    hooks.device = [&](const ffm_text_block &b) {
      check_rc(ffm_engine_idcount_add_device(ct.s, static_cast<int32_t>(b.nnz), map.n_fields ? b.field : nullptr, b.feat),
               "ffm_engine_idcount_add_device");
    };
    hooks.host = [&](const CsrPart &p) {
      check_rc(ffm_engine_idcount_add(ct.s, static_cast<int32_t>(p.feat.size()), map.n_fields ? p.field.data() : nullptr, p.feat.data(), 0),
               "ffm_engine_idcount_add");
    };
    hooks.sync = [&] { check_rc(ffm_engine_idcount_read(ct.s, nullptr, nullptr, nullptr), "ffm_engine_idcount_read"); };
    map.rows = device_parse_pass(opt, hooks);
  } else {
    CountBlock cb;  // (no page-locked memory to be had: the counter copies each block into its own)
    CsrStream stream(opt.train_path, opt.file_type, opt.thread_num);
    for (;;) {
      const size_t got = stream.next(kCountRows, cb.blk, kCountNnz, true);
      if (got == 0) break;
      map.rows += got;
      check_rc(ffm_engine_idcount_add(ct.s, static_cast<int32_t>(cb.blk.feat.size()), map.n_fields ? cb.blk.field.data() : nullptr,
                                      cb.blk.feat.data(), cb.pinned ? 1 : 0),
               "ffm_engine_idcount_add");
    }
  }
  int64_t n_valid = 0, n_bad = 0, kept = 0, folded = 0;
  check_rc(ffm_engine_idcount_read(ct.s, nullptr, &n_valid, &n_bad), "ffm_engine_idcount_read");
  map.words.resize((static_cast<size_t>(1) << map.bits) / 64);
  check_rc(ffm_engine_idcount_keep(ct.s, map.min_count, map.words.data(), &kept, &folded), "ffm_engine_idcount_keep");
  map.kept_slots = static_cast<uint64_t>(kept);
  std::printf("rare ids: counted %llu rows (%lld entries, %lld erased) in %.4lf s; %lld of 2^%d slots kept at min_count %d, %lld entries folded\n",
              static_cast<unsigned long long>(map.rows), static_cast<long long>(n_valid + n_bad), static_cast<long long>(n_bad),
              std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), static_cast<long long>(kept), map.bits,
              map.min_count, static_cast<long long>(folded));
  return map;
}

void resolve_rare_ids(config_options &opt) {
  RareIds map;
  if (opt.min_count > 1) map = count_rare_ids(opt);
  else if (!opt.rare_ids.empty()) map = read_rare_ids(opt.rare_ids.substr(1), model_fields(opt), opt.rare_bits);
  else return;
  if (!opt.rare_ids_out.empty()) write_rare_ids(opt.rare_ids_out, map);
  opt.rare_map_bits = map.bits;
  opt.rare_words = std::move(map.words);
}

}  // namespace ftrl
