// field_importance.h -- --field_importance true: which fields earn their place?  After the run's last
// evaluation the eval file is streamed once more through FtrlModel::predict_ablated_block (include/ffm_engine.h
// "Field ablation": the loss and AUC of the same model without each field, all from one pass), block by block
// through the synchronous call; the per-variant loss sums are added on the host in block order.  Prints
//   field importance: R rows, loss L[, auc A]
//   field f: without it loss L (delta D)[, auc A (delta D)]      one line per field, in field order
// (delta = without the field minus with it; the AUC parts only with --metrics auc).
#pragma once
#include <memory>

#include "cmd_option.h"
#include "csr_stream.h"
#include "ftrl_model.h"

namespace ftrl {

class FieldImportance {
 public:
  FieldImportance(const config_options &opt, FtrlModel *model);
  ~FieldImportance();
  void run();  // one pass over the eval file, then the lines

 private:
  FtrlModel *model_;
  std::unique_ptr<CsrStream> stream_;
  int batch_, n_fields_;
  bool want_auc_;
};

}  // namespace ftrl
