#include "field_importance.h"

#include <algorithm>
#include <cstdio>
#include <vector>

namespace ftrl {

FieldImportance::FieldImportance(const config_options &opt, FtrlModel *model)
    : model_(model), stream_(std::make_unique<CsrStream>(opt.eval_path, opt.file_type, opt.thread_num)),
      batch_(std::max(1, opt.batch_size)), n_fields_(opt.n_fields), want_auc_(opt.metrics == "auc") {}
FieldImportance::~FieldImportance() = default;

void FieldImportance::run() {
  model_->enable_ablation(want_auc_);
  std::vector<double> loss(static_cast<size_t>(n_fields_) + 1, 0.0);
  CsrBlock blk;
  unsigned long long rows = 0;
  for (;;) {
    const size_t got = stream_->next(static_cast<size_t>(batch_), blk);
    if (got == 0) break;
    model_->predict_ablated_block(blk, loss);
    rows += got;
  }
  stream_->rewind();
  const double n = rows ? static_cast<double>(rows) : 1.0;
  std::vector<ffm_metrics> auc;
  if (want_auc_) auc = model_->read_ablation_metrics(true);
  const size_t whole = static_cast<size_t>(n_fields_);
  std::printf("field importance: %llu rows, loss %.6lf", rows, loss[whole] / n);
  if (want_auc_) std::printf(", auc %.6lf", auc[whole].auc);
  std::printf("\n");
  for (size_t f = 0; f < whole; f++) {
    std::printf("field %zu: without it loss %.6lf (delta %+.6lf)", f, loss[f] / n, (loss[f] - loss[whole]) / n);
    if (want_auc_) std::printf(", auc %.6lf (delta %+.6lf)", auc[f].auc, auc[f].auc - auc[whole].auc);
    std::printf("\n");
  }
}

}  // namespace ftrl
