// plda_amd/csrc/layout.hpp -- one list of arrays gives both the bytes to reserve and each array's pointer (plain C++17, no
// HIP).  A site writes its list once, as a function of a Layout, and runs it twice: without a base (the sizing pass: every
// pointer nullptr, `end` the size) and, after the reserve, on the buffer (common.hpp: carve() does both).  Arrays lie in list
// order, each at a multiple of max(alignof(T), 16, align) bytes; an empty array takes no space and its pointer is never to be
// dereferenced; trailing slack is an entry of the list.  A size beyond size_t clears `ok` instead of wrapping.
#pragma once

#include <cstddef>
#include <cstdint>

namespace plda {

struct Layout {
  char *base = nullptr;   // nullptr: the sizing pass
  size_t end = 0;         // bytes laid out so far
  bool ok = true;

  template <typename T> Layout &take(T *&p, size_t n, size_t align = 16) {
    p = nullptr;
    if (align < 16) align = 16;
    if (align < alignof(T)) align = alignof(T);
    const size_t pad = (align - end % align) % align;
    if (pad > SIZE_MAX - end || n > (SIZE_MAX - end - pad) / sizeof(T)) { ok = false; return *this; }
    if (base && ok) p = reinterpret_cast<T *>(base + end + pad);
    if (n) end += pad + n * sizeof(T);
    return *this;
  }
  Layout &slack(size_t bytes) {
    if (bytes > SIZE_MAX - end) ok = false;
    else end += bytes;
    return *this;
  }
};

}  // namespace plda
