// count_pass.h -- the one pass over the training file that the counting pre-passes share (field_count.cpp,
// rare_count.cpp, value_count.cpp), before a model exists: the parser's threads fill a page-locked block and the
// device counts its entries straight from there (the host does nothing per entry) -- or, with --device_parse true, the
// file goes up as raw bytes and is parsed on the device into the arrays the counting object reads in HBM.
#pragma once
#include <functional>
#include <stdexcept>
#include <string>

#include "../../include/ffm_engine.h"
#include "cmd_option.h"

namespace ftrl {

inline void check_rc(int rc, const char *what) {
  if (rc != FFM_OK) throw std::runtime_error(std::string(what) + ": " + ffm_engine_last_error());
}

// Owns a counting object of the engine library.
template <class T, void (*Destroy)(T *)>
struct CountHandle {
  T *s = nullptr;
  ~CountHandle() { Destroy(s); }
};

// What a pass does with the entries of a block: the counting object's entry points, checked.
struct CountPass {
  bool with_val = false;  // the object reads values: the block's val array is page-locked too
  std::function<void(int32_t nnz, const int32_t *field, const int32_t *feat, const float *val)> add_device;  // *_add_device
  std::function<void(int32_t nnz, const int32_t *field, const int32_t *feat, const float *val, int zero_copy)> add;  // *_add
  std::function<void()> sync;  // back once the counting object has read what it was handed (*_read of nothing)
};

// One pass over opt.train_path, every block handed over in file order.  Returns the rows.
unsigned long long count_pass(const config_options &opt, const CountPass &pass);

}  // namespace ftrl
