#include "count_pass.h"

#include "count_block.h"
#include "text_stream.h"

namespace ftrl {

unsigned long long count_pass(const config_options &opt, const CountPass &pass) {
  if (opt.device_parse) {
    DeviceParseHooks hooks;
    hooks.device = [&](const ffm_text_block &b) { pass.add_device(static_cast<int32_t>(b.nnz), b.field, b.feat, b.val); };
    hooks.host = [&](const CsrPart &p) { pass.add(static_cast<int32_t>(p.feat.size()), p.field.data(), p.feat.data(), p.val.data(), 0); };
    hooks.sync = pass.sync;
    return device_parse_pass(opt, hooks);
  }
  unsigned long long rows = 0;
  CountBlock cb(pass.with_val);  // (no page-locked memory to be had: the counting object copies each block into its own)
  CsrStream stream(opt.train_path, opt.file_type, opt.thread_num);
  for (;;) {
    const size_t got = stream.next(kCountRows, cb.blk, kCountNnz, true);
    if (got == 0) break;
    rows += got;
    pass.add(static_cast<int32_t>(cb.blk.feat.size()), cb.blk.field.data(), cb.blk.feat.data(), cb.blk.val.data(), cb.pinned ? 1 : 0);
  }
  return rows;
}

}  // namespace ftrl
