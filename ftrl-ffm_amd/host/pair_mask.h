// pair_mask.h -- --pair_keep N --pair_mask_out FILE, --pair_mask @FILE: from measuring pairs to serving without them
// (include/ffm_engine.h "Pair masks").  What is here needs neither the engine nor a device: the selection rule, the
// words of a mask, and the mask file.
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

// keep[n_fields] of ffm_engine_set_pair_mask: bit g of word f and bit f of word g for every pair.
std::vector<uint64_t> pair_mask_words(int n_fields, const PairList &pairs);

void write_pair_mask(const std::string &path, int n_fields, const PairList &pairs);  // throws std::runtime_error
PairList read_pair_mask(const std::string &path, int n_fields);                      // throws std::invalid_argument

}  // namespace ftrl
