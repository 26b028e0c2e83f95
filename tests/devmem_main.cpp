// devmem_main.cpp -- csrc/rt_devmem.h over a fake backend (malloc / free plus live counters, the k-th
// allocation can be made to fail), built with ASan + UBSan and run by tests/test_devmem_cpu.py.
// Exit status 0: every check held and the sanitizers saw nothing.
#include <cstdio>
#include <cstdlib>

#include "rt_devmem.h"

namespace {
long g_live = 0, g_bytes = 0, g_allocs = 0, g_frees = 0, g_waits = 0;
long g_fail_at = -1; // the allocation call with this number (counted from 0 by g_allocs) fails
int g_failures = 0;

#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      g_failures++;                                                       \
    }                                                                     \
  } while (0)

long calls() { return g_allocs + g_frees + g_waits; }

struct Block { // a plain struct of raw pointers passed by value, like the kernels' parameter blocks
  int32_t *ids;
  const float *table;
  int n;
};
} // namespace

void *esc::devmem_allocate(size_t bytes) {
  if (g_allocs++ == g_fail_at) return nullptr;
  g_live++;
  g_bytes += (long)bytes;
  return std::malloc(bytes);
}

void esc::devmem_free(void *p, size_t bytes) {
  g_frees++;
  g_live--;
  g_bytes -= (long)bytes;
  std::free(p);
}

bool esc::devmem_wait(void *owner) {
  CHECK(owner == &g_waits);
  g_waits++;
  return true;
}

int main() {
  uint64_t epoch = 0;
  bool capturing = false;
  {
    esc::DevMem m(&g_waits, &epoch, &capturing);
    // alloc, alloc smaller, alloc 0: live count and bytes follow exactly
    double *a = nullptr;
    CHECK(m.alloc(a, 100) == ESC_OK && a && g_live == 1 && g_bytes == 800);
    CHECK(epoch == 0); // a first allocation ends no recording
    a[99] = 1.0;
    CHECK(m.alloc(a, 10) == ESC_OK && a && g_live == 1 && g_bytes == 80 && epoch == 1);
    CHECK(m.alloc(a, 0) == ESC_OK && !a && g_live == 0 && g_bytes == 0 && epoch == 2);
    CHECK(m.alloc(a, 0) == ESC_OK && !a && epoch == 2); // nothing held, nothing freed

    // grow: the first one from null allocates without ending a recording; below capacity nothing happens
    int32_t *g = nullptr;
    size_t cap = 0;
    CHECK(m.grow(g, cap, 64) == ESC_OK && g && cap == 64 && g_live == 1 && g_bytes == 256 && epoch == 2);
    g[63] = 7;
    int32_t *const g0 = g;
    long c0 = calls();
    CHECK(m.grow(g, cap, 64) == ESC_OK && m.grow(g, cap, 1) == ESC_OK && m.grow(g, cap, 0) == ESC_OK);
    CHECK(g == g0 && cap == 64 && calls() == c0 && epoch == 2);
    // above capacity: waits, frees, allocates; the epoch moves exactly once
    const long w0 = g_waits;
    CHECK(m.grow(g, cap, 65) == ESC_OK && g && cap == 65 && g_waits == w0 + 1 && epoch == 3);
    CHECK(g_live == 1 && g_bytes == 260);
    g[64] = 8;

    // a failed allocation inside grow: pointer null, capacity 0, the error code; the retry succeeds
    g_fail_at = g_allocs;
    CHECK(m.grow(g, cap, 1000) == ESC_ERR_HIP && !g && cap == 0 && g_live == 0 && g_bytes == 0);
    CHECK(epoch == 4); // the old buffer is gone
    CHECK(m.grow(g, cap, 1000) == ESC_OK && g && cap == 1000 && g_live == 1 && g_bytes == 4000 && epoch == 4);
    g[999] = 9;
    g_fail_at = g_allocs;
    CHECK(m.alloc(a, 5) == ESC_ERR_HIP && !a && g_live == 1);
    g_fail_at = -1;
    CHECK(m.alloc(a, 5) == ESC_OK && a && g_live == 2 && g_bytes == 4040);

    // inside a capture: the error, no backend call, pointer, capacity and epoch untouched
    capturing = true;
    const uint64_t e0 = epoch;
    double *const a0 = a;
    int32_t *const g1 = g;
    c0 = calls();
    CHECK(m.alloc(a, 50) == ESC_ERR_HIP && m.alloc(a, 0) == ESC_ERR_HIP && m.release(a) == ESC_ERR_HIP);
    CHECK(m.grow(g, cap, 2000) == ESC_ERR_HIP);
    CHECK(m.grow(g, cap, 1000) == ESC_OK); // within capacity nothing is rebuilt: fine inside a capture
    CHECK(a == a0 && g == g1 && cap == 1000 && epoch == e0 && calls() == c0 && m.refused() == 4);
    capturing = false;

    // release frees one pointer and ends the recordings; a null pointer is nothing
    CHECK(m.release(a) == ESC_OK && !a && g_live == 1 && epoch == e0 + 1);
    CHECK(m.release(a) == ESC_OK && epoch == e0 + 1);

    // pointers inside a plain struct, copied by value, and one through the `const T *&` overload
    Block b{nullptr, nullptr, 3};
    CHECK(m.alloc(b.ids, 12) == ESC_OK && m.alloc(b.table, 6) == ESC_OK && b.ids && b.table);
    CHECK(g_live == 3 && g_bytes == 4000 + 48 + 24);
    Block copy = b; // what a launch takes; the owner still frees the originals, once
    CHECK(copy.ids == b.ids && copy.table == b.table);
    CHECK(m.alloc(b.table, 7) == ESC_OK && g_bytes == 4000 + 48 + 28);
    CHECK(m.release(b.table) == ESC_OK && !b.table && g_live == 2);
    CHECK(m.alloc(b.table, 6) == ESC_OK && g_live == 3);
  } // g, b.ids and b.table are still held here
  CHECK(g_live == 0 && g_bytes == 0 && g_allocs - 2 == g_frees); // two allocations failed

  // the call-memory flavour has no epoch and no capture flag, and never looks for one
  {
    esc::DevMem m(&g_waits);
    float *p = nullptr;
    size_t cap = 0;
    CHECK(m.grow(p, cap, 8) == ESC_OK && m.grow(p, cap, 16) == ESC_OK && cap == 16 && g_live == 1);
    p[15] = 1.f;
    uint8_t *q = nullptr;
    CHECK(m.alloc(q, 3) == ESC_OK && m.alloc(q, 4) == ESC_OK && m.release(q) == ESC_OK && !q);
    CHECK(m.alloc(q, 5) == ESC_OK && g_live == 2 && m.refused() == 0);
    m.release_all();
    CHECK(g_live == 0 && g_bytes == 0);
    q = nullptr; // release_all leaves the callers' pointers alone: the context is about to die
    CHECK(m.alloc(q, 2) == ESC_OK && g_live == 1);
  }
  CHECK(g_live == 0 && g_bytes == 0);
  std::printf("failures=%d\n", g_failures);
  return g_failures ? 1 : 0;
}
