// field_ranges.h -- the fields' id ranges of an FFM model as the CLI handles them: the uniform rule, the
// file format of --field_ranges @FILE / --field_ranges_out (n_fields + 1 ascending integers, one per line),
// and the counting pass of --field_ranges counted (include/ffm_engine.h "Field sketches").
// The reference has no counterpart: its ids are laid out by whoever made the data (python/generate_data.py).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "cmd_option.h"

namespace ftrl {

// field f owns [f * (n_feats / n_fields), ...), the last field the rest (what FtrlModel has always built)
std::vector<int32_t> uniform_field_ranges(int n_fields, int n_feats);

// Reads and checks a ranges file: n_fields + 1 ascending integers, the first 0, the last n_feats, one per line
// (blank lines are skipped); hashed: every width at least 1.  Throws std::invalid_argument("file:line: ...").
std::vector<int32_t> read_field_ranges(const std::string &path, int n_fields, int n_feats, bool hashed);

// One integer per line.  Throws std::runtime_error when the file cannot be written.
void write_field_ranges(const std::string &path, const std::vector<int32_t> &field_start);

// --field_ranges counted (field_count.cpp; needs the engine library and a GPU): streams opt.train_path once
// through CsrStream, feeds every block's field / feat arrays to a sketch from page-locked memory, and turns
// the estimates into ranges (ffm_engine_field_ranges).  Prints the per-field lines and the summary line.
std::vector<int32_t> count_field_ranges(const config_options &opt);

// What main.cpp calls before a model exists: fills opt.field_start for counted / @FILE and writes
// --field_ranges_out.  Every other spelling leaves opt as it is.
void resolve_field_ranges(config_options &opt);

}  // namespace ftrl
