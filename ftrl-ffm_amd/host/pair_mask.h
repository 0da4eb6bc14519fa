// pair_mask.h -- --pair_keep N --pair_mask_out FILE, --pair_mask @FILE: from measuring pairs to serving without them
// (include/ffm_engine.h "Pair masks").  What is here needs neither the engine nor a device: the selection rule, the
// words of a mask, and the mask file.
//
// --pair_curve LIST|auto, --pair_loss_budget T: the same ranking as a ladder of nested masks -- one more pass gives
// the loss of "keep the best N" for every listed N (trainer.h: run_pair_curve), and the budget picks the N to write.
//
// The selection rule, after the pair importance pass: rank all V = pair_count(n_fields) pairs by
//   delta = loss without the pair - loss of the rows
// (both the doubles the pass has), largest first, ties to the lower pair index, and keep the first N.  A delta that
// is not finite ends the run: `pair mask: loss without pair f g is not finite`.
//
// The file is small text:
//   ffm-pair-mask 1 <n_fields> <n_kept>
//   f g              one line per kept pair, f <= g, the pair index ascending
// The reader checks the magic, the version, n_fields against the run's, the count, the ranges, the order and
// duplicates; every message starts with the path.
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace ftrl {

using PairList = std::vector<std::pair<int, int>>;  // (f, g) with f <= g, the pair index ascending

// The first n_keep pairs of the ranking above.  loss: V + 1 sums, the rows' own last.  Throws std::invalid_argument
// for n_fields outside [1, 64], another length or n_keep outside [0, V]; std::runtime_error for a delta that is not
// finite.  *smallest_kept (may be null): the delta of the last pair kept, 0 when none is.
PairList select_pairs(int n_fields, const std::vector<double> &loss, int n_keep, double *smallest_kept = nullptr);

// The ranking itself: all V pair indices, best first (the rule above; the same throws).  select_pairs keeps its first
// n_keep.
std::vector<int> rank_pairs(int n_fields, const std::vector<double> &loss);

// --pair_curve: the level table of include/ffm_engine.h "Pruning curve" for that ranking -- level[f][g] = level[g][f] =
// the position of pair (f, g) in `order` (a permutation of the V pair indices), row-major [n_fields][n_fields] -- so
// that cut N is "keep the best N pairs", the pairs select_pairs(.., N) returns.
std::vector<uint16_t> pair_curve_levels(int n_fields, const std::vector<int> &order);

// --pair_loss_budget T: the position in `keep` (ascending numbers of pairs) of the smallest N whose per-row loss
// delta (curve_loss[i] - curve_loss.back()) / rows is <= budget, or -1 when none is.  curve_loss: one sum per listed
// N, the rows' own last.  A delta that is not finite meets no budget.
int pick_by_budget(const std::vector<int> &keep, const std::vector<double> &curve_loss, unsigned long long rows, double budget);

// keep[n_fields] of ffm_engine_set_pair_mask: bit g of word f and bit f of word g for every pair.
std::vector<uint64_t> pair_mask_words(int n_fields, const PairList &pairs);

void write_pair_mask(const std::string &path, int n_fields, const PairList &pairs);  // throws std::runtime_error
PairList read_pair_mask(const std::string &path, int n_fields);                      // throws std::invalid_argument

}  // namespace ftrl
