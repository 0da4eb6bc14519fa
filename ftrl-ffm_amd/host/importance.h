// importance.h -- --field_importance true, --pair_importance true: which fields earn their place, which
// interactions carry the model?  After the run's last evaluation the eval file is streamed once more per flag
// (fields first) through FtrlModel::predict_ablated_block (include/ffm_engine.h "Field ablation", "Pair ablation": the
// loss and AUC of the same model without each field, or without the terms between fields f and g for every pair
// f <= g, all from one pass), block by block through the synchronous call; the per-variant loss sums are added on
// the host in block order (trainer.h: run_importance).  What is here needs neither the engine nor a device: the
// numbering of the pairs, the histogram memory the pairs' AUC parts cost, and the lines
//   field importance: R rows, loss L[, auc A]
//   field f: without it loss L (delta D)[, auc A (delta D)]      one line per field, in field order
// and
//   pair importance: R rows, loss L[, auc A]
//   pair f g: without it loss L (delta D)[, auc A (delta D)]     one line per pair whose loss sum differs from the
//                                                                 whole row's, in index order
//   pair importance: P of V pairs listed, Q never changed a row
// (delta = without the field or pair minus with it; the AUC parts only with --metrics auc).  A pair that no row of
// the file has -- or whose terms are all zero -- has the whole row's loss sum bit for bit and is counted, not listed.
#pragma once
#include <cstdio>
#include <vector>

#include "../../include/ffm_engine.h"

namespace ftrl {

// The numbering of include/ffm_engine.h "Pair ablation" (ffm_engine_pair_count / _pair_index restated: this file
// links without the engine).  f <= g.
inline int pair_count(int n_fields) { return n_fields * (n_fields + 1) / 2; }
inline int pair_index(int n_fields, int f, int g) { return f * n_fields - f * (f - 1) / 2 + (g - f); }

// Bytes of device memory the V + 1 score histograms of --metrics auc take.
unsigned long long pair_histogram_bytes(int n_fields);
// `pair importance: V + 1 score histograms, B bytes of device memory` -- printed before they are allocated.
void print_pair_histogram_memory(std::FILE *out, int n_fields);
// The lines above.  loss: the variants' loss sums over `rows` rows, n_fields + 1 of them for the fields and V + 1 for
// the pairs, the rows themselves last; auc: null, or as many variants' metrics.  Return -1, with nothing printed,
// when a length is another; otherwise the number of lines per field or pair.
int print_field_importance(std::FILE *out, int n_fields, unsigned long long rows, const std::vector<double> &loss,
                           const std::vector<ffm_metrics> *auc);
int print_pair_importance(std::FILE *out, int n_fields, unsigned long long rows, const std::vector<double> &loss,
                          const std::vector<ffm_metrics> *auc);
// --pair_curve (include/ffm_engine.h "Pruning curve"):
//   pair curve: R rows, loss L[, auc A]
//   keep N of V pairs: loss L (delta D)[, auc A (delta D)]       one line per listed N, ascending
// keep: the listed N; loss / auc: one per listed N, the rows themselves last.  Returns the lines per N, or -1 with
// nothing printed when a length is another.
int print_pair_curve(std::FILE *out, int n_fields, unsigned long long rows, const std::vector<int> &keep, const std::vector<double> &loss,
                     const std::vector<ffm_metrics> *auc);

}  // namespace ftrl
