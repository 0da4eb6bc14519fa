// rare_count.cpp -- --min_count T: one pass over the training file before a model exists (count_pass.h).  The
// device counts the hashed slot of the (field, feat) entries, one small kernel turns the counts into the keep-map.
// With --field_ranges counted the file is then streamed once more through a FILTERED sketch (count_field_ranges),
// so that the ranges are sized by the ids that stay.
#include <chrono>
#include <cstdio>
#include <stdexcept>

#include "count_pass.h"
#include "rare_ids.h"

namespace ftrl {

namespace {

int model_fields(const config_options &opt) { return opt.model_type == "FFM" ? opt.n_fields : 0; }

}  // namespace

RareIds count_rare_ids(const config_options &opt) {
  const auto t0 = std::chrono::steady_clock::now();
  RareIds map;
  map.bits = opt.rare_bits ? opt.rare_bits : default_rare_bits(opt.n_feats);
  map.min_count = opt.min_count;
  map.n_fields = model_fields(opt);
  CountHandle<ffm_idcount, ffm_engine_idcount_destroy> ct;
  {
    const int rc = ffm_engine_idcount_create(map.n_fields, map.bits, map.min_count, opt.device, &ct.s);
    if (rc == FFM_E_INVALID) throw std::invalid_argument(std::string("--min_count: ") + ffm_engine_last_error());
    check_rc(rc, "ffm_engine_idcount_create");
  }
  CountPass pass;
  pass.add_device = [&](int32_t nnz, const int32_t *field, const int32_t *feat, const float *) {
    check_rc(ffm_engine_idcount_add_device(ct.s, nnz, map.n_fields ? field : nullptr, feat), "ffm_engine_idcount_add_device");
  };
  pass.add = [&](int32_t nnz, const int32_t *field, const int32_t *feat, const float *, int zero_copy) {
    check_rc(ffm_engine_idcount_add(ct.s, nnz, map.n_fields ? field : nullptr, feat, zero_copy), "ffm_engine_idcount_add");
  };
  pass.sync = [&] { check_rc(ffm_engine_idcount_read(ct.s, nullptr, nullptr, nullptr), "ffm_engine_idcount_read"); };
  map.rows = count_pass(opt, pass);
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
