// locked_pages.h -- arrays in pages that the device's runtime allocated page-locked (ffm_engine_alloc_host).
// Not every system lets the runtime lock pages somebody else allocated (ffm_engine_pin_host then fails), so
// whatever the device is to read or write in place is moved into such pages BEFORE it is page-locked:
// ffm_engine_pin_host finds nothing left to do there, and still locks in place what could not be moved.
#pragma once
#include <new>

#include "../../include/ffm_engine.h"
#include "types.h"

namespace ftrl {

inline const PageSource *locked_pages() {
  static const PageSource source{
      [](size_t bytes) -> void * {
        void *p = nullptr;
        return ffm_engine_alloc_host(&p, bytes) == FFM_OK ? p : nullptr;
      },
      [](void *p) { ffm_engine_free_host(p); }};
  return &source;
}

// v's storage, `capacity` elements of it, in pages allocated page-locked; its elements stay.
// false: none to be had -- v is as it was (in the heap's pages).
template <typename V>
bool to_locked_pages(V &v, size_t capacity) {
  try {
    const typename V::allocator_type from_locked(locked_pages());
    V locked(from_locked);
    locked.reserve(capacity > v.size() ? capacity : v.size());
    locked.assign(v.begin(), v.end());
    v = std::move(locked);
    return true;
  } catch (const std::bad_alloc &) {
    return false;
  }
}

}  // namespace ftrl
