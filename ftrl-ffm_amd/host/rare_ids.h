// rare_ids.h -- --min_count / --rare_bits / --rare_ids @FILE / --rare_ids_out (include/ffm_engine.h "Rare ids"):
// the keep-map every engine of a run folds rare ids by, counted on the device from the training file or read from
// the file an earlier run wrote.  The map is not in checkpoints, exactly as the fields' ranges are not: a resumed,
// scoring or serving run passes --rare_ids @FILE.
//
// File: 8 bytes of magic, then little-endian: a 32-bit version, bits, min_count, n_fields (0: LR / FM), the 64-bit
// rows counted, kept slots and checksum of the words (kRareIdsHeaderBytes), then ONE zstd frame of the 2^bits / 64
// words as 32-bit halves, low half first -- the frames of persist.h, as serve_delta.h uses them.
// rare_ids.cpp knows nothing of the engine; the counting pass and resolve_rare_ids are rare_count.cpp.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "cmd_option.h"

namespace ftrl {

struct RareIds {
  int bits = 0, min_count = 0, n_fields = 0;  // n_fields 0: LR / FM
  uint64_t rows = 0, kept_slots = 0;
  std::vector<uint64_t> words;  // [2^bits / 64]
};
constexpr size_t kRareIdsHeaderBytes = 48;
constexpr uint32_t kRareIdsVersion = 1;

// --rare_bits' default: the smallest B with 2^B >= 4 * n_feats, inside [16, 30].
int default_rare_bits(int n_feats);
// FNV-1a over the words, a word at a time.
uint64_t rare_ids_checksum(const std::vector<uint64_t> &words);
// Throws std::invalid_argument when the map is not one (bits outside [8, 30], words of another length).
void write_rare_ids(const std::string &path, const RareIds &map);
// Reads and checks the whole file.  n_fields: the model's (0: LR / FM); bits: what --rare_bits asked for, 0 = whatever
// the file holds.  Throws std::invalid_argument, with the path in the message, on a file that cannot be opened, a
// wrong magic or version, a truncated header or frame, a frame whose length is not the header's 2^bits / 64 words, a
// wrong checksum, a kept-slots count that is not the words', another n_fields, other bits.
RareIds read_rare_ids(const std::string &path, int n_fields, int bits);

// --min_count T: one pass over --train_data through a device counter (cap T), the keep-map of T, the line
// `rare ids: counted ...`.  (rare_count.cpp; needs a device.)
RareIds count_rare_ids(const config_options &opt);
// What main.cpp calls before resolve_field_ranges: fills opt.rare_map_bits / opt.rare_words from --min_count or
// --rare_ids @FILE and writes --rare_ids_out.  Nothing asked for: nothing done.
void resolve_rare_ids(config_options &opt);

}  // namespace ftrl
