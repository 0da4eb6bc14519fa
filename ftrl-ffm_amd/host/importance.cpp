#include "importance.h"

namespace ftrl {

unsigned long long pair_histogram_bytes(int n_fields) {
  // per variant: positives and negatives per bin, and the count of NaN scores, 64 bits each
  const unsigned long long words = 2ull * FFM_METRIC_BINS + 1ull;
  return (static_cast<unsigned long long>(pair_count(n_fields)) + 1ull) * words * 8ull;
}

void print_pair_histogram_memory(std::FILE *out, int n_fields) {
  std::fprintf(out, "pair importance: %d score histograms, %llu bytes of device memory\n", pair_count(n_fields) + 1,
               pair_histogram_bytes(n_fields));
}

int print_field_importance(std::FILE *out, int n_fields, unsigned long long rows, const std::vector<double> &loss,
                           const std::vector<ffm_metrics> *auc) {
  const size_t whole = static_cast<size_t>(n_fields);
  if (loss.size() != whole + 1 || (auc && auc->size() != whole + 1)) return -1;
  const double n = rows ? static_cast<double>(rows) : 1.0;
  std::fprintf(out, "field importance: %llu rows, loss %.6lf", rows, loss[whole] / n);
  if (auc) std::fprintf(out, ", auc %.6lf", (*auc)[whole].auc);
  std::fprintf(out, "\n");
  for (size_t f = 0; f < whole; f++) {
    std::fprintf(out, "field %zu: without it loss %.6lf (delta %+.6lf)", f, loss[f] / n, (loss[f] - loss[whole]) / n);
    if (auc) std::fprintf(out, ", auc %.6lf (delta %+.6lf)", (*auc)[f].auc, (*auc)[f].auc - (*auc)[whole].auc);
    std::fprintf(out, "\n");
  }
  return n_fields;
}

int print_pair_importance(std::FILE *out, int n_fields, unsigned long long rows, const std::vector<double> &loss,
                          const std::vector<ffm_metrics> *auc) {
  const int V = pair_count(n_fields);
  const size_t whole = static_cast<size_t>(V);
  if (loss.size() != whole + 1 || (auc && auc->size() != whole + 1)) return -1;
  const double n = rows ? static_cast<double>(rows) : 1.0;
  std::fprintf(out, "pair importance: %llu rows, loss %.6lf", rows, loss[whole] / n);
  if (auc) std::fprintf(out, ", auc %.6lf", (*auc)[whole].auc);
  std::fprintf(out, "\n");
  int listed = 0;
  for (int f = 0; f < n_fields; f++)
    for (int g = f; g < n_fields; g++) {
      const size_t v = static_cast<size_t>(pair_index(n_fields, f, g));
      if (loss[v] == loss[whole]) continue;  // (no row's sum moved by a bit: counted below)
      std::fprintf(out, "pair %d %d: without it loss %.6lf (delta %+.6lf)", f, g, loss[v] / n, (loss[v] - loss[whole]) / n);
      if (auc) std::fprintf(out, ", auc %.6lf (delta %+.6lf)", (*auc)[v].auc, (*auc)[v].auc - (*auc)[whole].auc);
      std::fprintf(out, "\n");
      listed++;
    }
  std::fprintf(out, "pair importance: %d of %d pairs listed, %d never changed a row\n", listed, V, V - listed);
  return listed;
}

int print_pair_curve(std::FILE *out, int n_fields, unsigned long long rows, const std::vector<int> &keep, const std::vector<double> &loss,
                     const std::vector<ffm_metrics> *auc) {
  const size_t whole = keep.size();
  if (loss.size() != whole + 1 || (auc && auc->size() != whole + 1)) return -1;
  const double n = rows ? static_cast<double>(rows) : 1.0;
  std::fprintf(out, "pair curve: %llu rows, loss %.6lf", rows, loss[whole] / n);
  if (auc) std::fprintf(out, ", auc %.6lf", (*auc)[whole].auc);
  std::fprintf(out, "\n");
  for (size_t i = 0; i < whole; i++) {
    std::fprintf(out, "keep %d of %d pairs: loss %.6lf (delta %+.6lf)", keep[i], pair_count(n_fields), loss[i] / n, (loss[i] - loss[whole]) / n);
    if (auc) std::fprintf(out, ", auc %.6lf (delta %+.6lf)", (*auc)[i].auc, (*auc)[i].auc - (*auc)[whole].auc);
    std::fprintf(out, "\n");
  }
  return static_cast<int>(whole);
}

}  // namespace ftrl
