// tests/layout_check/check.cpp -- host-only check of plda_amd/csrc/layout.hpp (tests/test_layout.py builds it with the
// address and undefined-behaviour sanitizers and runs it): the sizing pass and the pointer pass of one list agree, arrays are
// aligned, in list order and disjoint, empty arrays take no space, and a size beyond size_t is an error, not a wrap.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "layout.hpp"

using plda::Layout;

static int failures = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

struct alignas(16) Quad { int x, y, z, w; };   // (the size and alignment of the device's int4)

struct Arrays {
  int *a; Quad *q; double *d; float *none_mid; double *strong; char *tail; int *none_end;
  void lay(Layout &c) {
    c.take(a, 7);                    // 28 bytes: whatever follows needs padding
    c.take(q, 3).take(d, 5);         // 48 and 40 bytes
    c.take(none_mid, 0).take(strong, 3, 256).take(tail, 1).take(none_end, 0).slack(64);
  }
};

static uintptr_t addr(const void *p) { return reinterpret_cast<uintptr_t>(p); }

int main() {
  Arrays s;
  s.a = reinterpret_cast<int *>(&s);                                   // (stale: the sizing pass must clear it)
  Layout size;
  s.lay(size);
  CHECK(size.ok);
  CHECK(s.a == nullptr && s.q == nullptr && s.strong == nullptr);      // the sizing pass hands out nothing
  // 0..28 | 32..80 | 80..120 | 256..280 | 288..289 | + 64
  CHECK(size.end == 289 + 64);

  // an allocation of exactly that size, 256-aligned as device allocations are: the sanitizer sees any write outside it
  char *buf = static_cast<char *>(std::aligned_alloc(256, (size.end + 255) / 256 * 256));
  CHECK(buf != nullptr);
  Layout at{buf};
  s.lay(at);
  CHECK(at.ok && at.end == size.end);
  CHECK(addr(s.a) == addr(buf));
  CHECK(addr(s.q) % 16 == 0 && addr(s.d) % 16 == 0 && addr(s.tail) % 16 == 0);
  CHECK(addr(s.strong) % 256 == 0);
  // list order, no overlap
  CHECK(addr(s.a + 7) <= addr(s.q));
  CHECK(addr(s.q + 3) <= addr(s.d));
  CHECK(addr(s.d + 5) <= addr(s.strong));
  CHECK(addr(s.strong + 3) <= addr(s.tail));
  // an empty array takes no space: what follows lies where it would have lain without it
  CHECK(addr(s.none_mid) >= addr(s.d + 5) && addr(s.none_mid) <= addr(s.strong));
  CHECK(addr(s.strong) - addr(buf) == 256);
  CHECK(addr(s.none_end) >= addr(s.tail + 1));
  CHECK(addr(s.tail + 1) + 64 == addr(buf) + size.end);                // the last array ends at the total less the slack
  // every element is writable inside the allocation
  std::memset(s.a, 1, 7 * sizeof(int));
  std::memset(s.q, 2, 3 * sizeof(Quad));
  std::memset(s.d, 3, 5 * sizeof(double));
  std::memset(s.strong, 4, 3 * sizeof(double));
  s.tail[0] = 5;
  CHECK(s.a[6] == 0x01010101 && s.q[0].x == 0x02020202 && s.tail[0] == 5);
  std::free(buf);

  // overflow: of the product, of the running sum, of the slack -- and it stays an error
  double *pd = nullptr;
  char *pc = nullptr;
  Layout o1;
  CHECK(!o1.take(pd, SIZE_MAX / 4).ok && pd == nullptr);
  Layout o2;
  CHECK(o2.take(pc, SIZE_MAX - 40).ok);
  CHECK(!o2.take(pd, 8).ok);
  CHECK(!o2.take(pc, 1).ok);                                           // (it stays an error)
  Layout o3;
  CHECK(!o3.take(pc, 100).slack(SIZE_MAX - 50).ok);
  char one[16];
  Layout o4{one};
  pd = reinterpret_cast<double *>(one);
  CHECK(!o4.take(pd, SIZE_MAX / 8 + 1).ok && pd == nullptr);           // with a base too: no pointer from a wrapped size
  // an empty list
  Layout e;
  CHECK(e.ok && e.end == 0);

  if (failures) return 1;
  std::printf("layout ok\n");
  return 0;
}
