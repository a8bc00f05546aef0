// Stand-alone check of PbOwned (csrc/pb_memory.hpp) on the CPU: a malloc-backed trait that counts its blocks and fails
// on request.  Built with -fsanitize=address,undefined and run as a plain program by tests/test_memory_owner.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "pb_memory.hpp"

namespace {

struct HeapTraits {
  static constexpr bool counted = false;
  static inline long live = 0, allocs = 0, frees = 0;
  static inline bool failNext = false;
  static hipError_t alloc(void **p, size_t bytes) {
    if (failNext) {
      failNext = false;
      return hipErrorOutOfMemory;
    }
    *p = malloc(bytes ? bytes : 1);
    if (!*p) return hipErrorOutOfMemory;
    memset(*p, 0xA5, bytes);
    live++, allocs++;
    return hipSuccess;
  }
  static hipError_t free(void *p) {
    ::free(p);
    live--, frees++;
    return hipSuccess;
  }
};
using Buf = PbOwned<int, HeapTraits>;

int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAILED line %d: %s\n", __LINE__, #cond);           \
      failures++;                                                \
    }                                                            \
  } while (0)

}  // namespace

int main() {
  {
    Buf a;  // an empty owner is null
    CHECK(!a && a.get() == nullptr && a.capacity() == 0 && HeapTraits::live == 0);
    a.reset();
    CHECK(HeapTraits::frees == 0);

    // alloc holds `count` elements and frees the previous block
    CHECK(a.alloc(10) == hipSuccess && a && a.capacity() == 10 && HeapTraits::live == 1);
    a[9] = 7;  // (the last element is inside the block: the sanitizer watches)
    int *const first = a;
    CHECK(first == a.get() && *(a + 9) == 7);
    CHECK(a.alloc(20) == hipSuccess && a.capacity() == 20 && HeapTraits::live == 1);
    CHECK(HeapTraits::allocs == 2 && HeapTraits::frees == 1);
    a[19] = 1;

    // a failing alloc leaves the owner empty with capacity 0, the old block freed
    HeapTraits::failNext = true;
    CHECK(a.alloc(30) == hipErrorOutOfMemory && !a && a.capacity() == 0 && HeapTraits::live == 0);
    CHECK(HeapTraits::frees == 2);

    // ensure: allocates from empty, does nothing at sufficient capacity, reallocates above it
    CHECK(a.ensure(8) == hipSuccess && a.capacity() == 8 && HeapTraits::allocs == 3);
    int *const kept = a;
    kept[0] = 42;
    CHECK(a.ensure(8) == hipSuccess && a.ensure(3) == hipSuccess && a.ensure(0) == hipSuccess);
    CHECK(a.get() == kept && a[0] == 42 && a.capacity() == 8 && HeapTraits::allocs == 3 && HeapTraits::frees == 2);
    CHECK(a.ensure(9) == hipSuccess && a.capacity() == 9 && HeapTraits::allocs == 4 && HeapTraits::frees == 3);
    HeapTraits::failNext = true;
    CHECK(a.ensure(100) == hipErrorOutOfMemory && !a && a.capacity() == 0 && HeapTraits::live == 0);
    CHECK(a.ensure(0) == hipSuccess && !a && HeapTraits::allocs == 4);  // (nothing asked for, nothing held)

    // move construction, move assignment and swap leave exactly one owner per block
    CHECK(a.alloc(4) == hipSuccess);
    int *const pa = a;
    Buf b(std::move(a));
    CHECK(!a && a.capacity() == 0 && b.get() == pa && b.capacity() == 4 && HeapTraits::live == 1);
    Buf c;
    CHECK(c.alloc(6) == hipSuccess && HeapTraits::live == 2);
    int *const pc = c;
    c = std::move(b);  // c's block goes, b's moves in
    CHECK(!b && b.capacity() == 0 && c.get() == pa && c.capacity() == 4 && HeapTraits::live == 1);
    (void)pc;
    Buf &self = c;
    c = std::move(self);  // onto itself: still held, once
    CHECK(c.get() == pa && c.capacity() == 4 && HeapTraits::live == 1);
    CHECK(a.alloc(2) == hipSuccess && HeapTraits::live == 2);
    int *const pa2 = a;
    a.swap(c);
    CHECK(a.get() == pa && a.capacity() == 4 && c.get() == pa2 && c.capacity() == 2 && HeapTraits::live == 2);
    c = Buf();  // "off" is the assignment of a fresh value
    CHECK(!c && HeapTraits::live == 1);

    Buf pair[2];  // the ping-pong of the step loop
    CHECK(pair[0].alloc(3) == hipSuccess && pair[1].alloc(5) == hipSuccess);
    int *const p0 = pair[0], *const p1 = pair[1];
    pair[0].swap(pair[1]);
    CHECK(pair[0].get() == p1 && pair[1].get() == p0 && pair[0].capacity() == 5 && pair[1].capacity() == 3);
    CHECK(HeapTraits::live == 3);
  }
  // every owner is gone: the trait's live count is zero, and nothing was counted as device memory
  CHECK(HeapTraits::live == 0 && HeapTraits::allocs == HeapTraits::frees);
  CHECK(PbMemoryLive::buffers.load() == 0 && PbMemoryLive::bytes.load() == 0);
  if (failures) return 1;
  printf("pb_memory_check ok: %ld blocks\n", HeapTraits::allocs);
  return 0;
}
