// sample_weights.h -- per-row training weights of the CLI: --pos_weight / --neg_weight (a weight per
// class) and --weight_data (one decimal per row of --train_data, the libsvm-weights convention).
// The reference has no counterpart (its Sample is {x, y}, src/include/data/sample.h:6-9); click logs
// trained with down-sampled negatives (python/generate_data.py has the option) are corrected by an
// importance weight per row.  A row's weight is the fp32 product of its file weight and the weight of
// its class; the engine scales the row's gradient and loss term by it (include/ffm_engine.h "Sample
// weights").  Weights are not model state: nothing of them is written to any file, and a resumed run
// must be given the same flags.
#pragma once
#include <cstddef>
#include <string>
#include <vector>

#include "cmd_option.h"
#include "types.h"

namespace ftrl {

struct SampleWeights {
  bool on = false;            // one of the three flags was given: blocks carry a weight array
  float pos = 1.0f, neg = 1.0f;
  std::vector<float> file;    // [rows of --train_data] in file order, or empty
  float of(size_t row, int label) const {
    const float c = label > 0 ? pos : neg;
    return file.empty() ? c : file[row] * c;
  }
  // Fills blk.weight for the block's rows -- row j of the block is row idx[j] of the file, or
  // first + j when idx is null -- and returns the sum of the weights written, in double.
  double fill(CsrBlock &blk, const int *idx, size_t first) const;
};

// Rows of a libffm / libsvm text as the parsers count them: lines that hold anything but blanks.
size_t count_data_rows(const std::string &path);

// One decimal per line.  Throws std::runtime_error("<file>:<line>: ...") for a line that does not
// parse, a negative or a non-finite weight; blank lines are errors too (a weight file has exactly one
// line per row).
std::vector<float> read_weight_file(const std::string &path);

// What the flags ask for, checked in full before anything is trained: the class weights finite and
// >= 0 (std::invalid_argument), the file readable, well-formed and as long as --train_data has rows
// (std::runtime_error naming the file and the line).  Without any of the flags: `on` is false and
// nothing is read.
SampleWeights load_sample_weights(const config_options &opt);

}  // namespace ftrl
