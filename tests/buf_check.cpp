// buf_check.cpp -- stand-alone check of krepp_amd/csrc/kr_buf.h (tests/test_buf_host.py builds and runs it, with the address and
// undefined-behaviour sanitizers where they can be linked).  The policy below is malloc / free that can be told to fail its k-th
// allocation and counts the blocks alive; the scenario is run once without a failure to learn how many allocations it makes, then
// once for every k with that allocation failing.
#include "kr_buf.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>

namespace {

struct TestMem {
  static long calls, fail_at, live, live_at_alloc, peak;
  static size_t last_bytes;
  static void* alloc(size_t bytes)
  {
    ++calls;
    live_at_alloc = live;
    last_bytes = bytes;
    if (calls == fail_at) return nullptr;
    void* p = malloc(bytes);
    if (p && ++live > peak) peak = live;
    return p;
  }
  static void free(void* p)
  {
    --live;
    ::free(p);
  }
};
long TestMem::calls = 0, TestMem::fail_at = 0, TestMem::live = 0, TestMem::live_at_alloc = 0, TestMem::peak = 0;
size_t TestMem::last_bytes = 0;

template <class T>
using TBuf = Buf<T, TestMem>;
struct Pair { double a, b; };

#define CHECK(cond)                                                                                  \
  do {                                                                                               \
    if (!(cond)) {                                                                                   \
      fprintf(stderr, "buf_check: line %d (failing allocation %ld): %s\n", __LINE__, TestMem::fail_at, #cond); \
      exit(1);                                                                                       \
    }                                                                                                \
  } while (0)

template <class B>
bool empty(const B& b) { return b.get() == nullptr && b.size() == 0 && b.bytes() == 0; }

// One buffer: first allocation, reuse, growth, renewal, the 16-byte floor.
void single()
{
  TBuf<uint32_t> a;
  CHECK(empty(a));
  CHECK(a.reserve(0) && empty(a) && TestMem::calls == 0); // nothing asked for, nothing allocated
  bool ok = a.reserve(100);
  CHECK(TestMem::last_bytes == 400);
  CHECK(ok ? (a.get() && a.size() == 100 && a.bytes() == 400 && TestMem::live == 1) : (empty(a) && TestMem::live == 0));
  if (ok) { // at or below the size in hand: the same block, no allocation
    const long c0 = TestMem::calls;
    uint32_t* p0 = a.get();
    a.get()[99] = 7; // (the sanitizer watches the block's end)
    CHECK(a.reserve(100) && a.reserve(1) && a.reserve(0) && TestMem::calls == c0 && a.get() == p0 && a.size() == 100);
  }
  ok = a.reserve(1000); // growth: the old block is gone before the new one is asked for
  CHECK(TestMem::live_at_alloc == 0 && TestMem::last_bytes == 4000);
  CHECK(ok ? (a.size() == 1000 && TestMem::live == 1) : (empty(a) && TestMem::live == 0));
  if (ok) a.get()[999] = 7;
  const long c1 = TestMem::calls;
  ok = a.renew(1000); // the same size, unconditionally a new block
  CHECK(TestMem::calls == c1 + 1 && TestMem::live_at_alloc == 0);
  CHECK(ok ? (a.size() == 1000 && TestMem::live == 1) : (empty(a) && TestMem::live == 0));
  ok = a.reserve(1000); // (after a failed renewal this allocates again: an empty buffer has no capacity to go stale)
  CHECK(ok && a.get() && a.size() == 1000 && TestMem::live == 1);
  TBuf<char> c;
  ok = c.reserve(3); // never less than 16 bytes
  CHECK(TestMem::last_bytes == 16);
  CHECK(ok ? (c.size() == 3 && c.bytes() == 16) : empty(c));
  if (ok) c.get()[15] = 1;
  a.reset();
  CHECK(empty(a) && TestMem::live == (ok ? 1 : 0));
}

// Five buffers with one capacity: all of them or none, whichever member fails; growth holds no more than renewing them one by one.
void group()
{
  TBuf<uint32_t> b1;
  TBuf<double> b2;
  TBuf<uint8_t> b3;
  TBuf<Pair> b4;
  TBuf<uint64_t> b5;
  auto all_empty = [&] { return empty(b1) && empty(b2) && empty(b3) && empty(b4) && empty(b5); };
  auto all_hold = [&](size_t n) {
    return b1.get() && b2.get() && b3.get() && b4.get() && b5.get() && b1.size() >= n && b2.size() >= n && b3.size() >= n && b4.size() >= n && b5.size() >= n;
  };
  for (size_t n : {(size_t)64, (size_t)256}) { // first allocation, then growth
    const long live0 = TestMem::live; // 0, or the five blocks of the first round
    TestMem::peak = TestMem::live;
    if (!reserve_all(n, b1, b2, b3, b4, b5)) {
      CHECK(all_empty() && TestMem::live == 0);
      const long c0 = TestMem::calls;
      CHECK(reserve_all(n, b1, b2, b3, b4, b5)); // (only one allocation fails: this one is allowed)
      CHECK(TestMem::calls == c0 + 5);
    }
    // renewed one by one, member i is allocated while i - 1 new and 5 - i old blocks are held: never more than five alive
    CHECK(TestMem::peak <= 5 && TestMem::peak >= live0);
    CHECK(all_hold(n) && TestMem::live == 5);
    b4.get()[n - 1].b = 1.0, b3.get()[n - 1] = 1;
    const long c1 = TestMem::calls;
    CHECK(reserve_all(n / 2, b1, b2, b3, b4, b5) && TestMem::calls == c1 && all_hold(n)); // below the size: nothing happens
  }
}

// Moves and swaps: exactly one owner of every block.
void owners()
{
  TBuf<uint32_t> a, b;
  if (!a.reserve(10)) CHECK(empty(a) && a.reserve(10));
  if (!b.reserve(20)) CHECK(empty(b) && b.reserve(20));
  CHECK(TestMem::live == 2);
  uint32_t *pa = a.get(), *pb = b.get();
  a.swap(b);
  CHECK(a.get() == pb && a.size() == 20 && b.get() == pa && b.size() == 10 && TestMem::live == 2);
  {
    TBuf<uint32_t> m(std::move(a)); // move construction: the source is empty, the block alive
    CHECK(empty(a) && m.get() == pb && m.size() == 20 && TestMem::live == 2);
    b = std::move(m); // move assignment: the target's block is freed, the source empty
    CHECK(empty(m) && b.get() == pb && b.size() == 20 && TestMem::live == 1);
  }
  CHECK(TestMem::live == 1); // (the moved-from buffer's destructor freed nothing)
  b.get()[19] = 1;
}

long scenario(long fail_at)
{
  TestMem::calls = 0, TestMem::fail_at = fail_at, TestMem::live = 0, TestMem::live_at_alloc = 0, TestMem::peak = 0;
  single();
  CHECK(TestMem::live == 0);
  group();
  CHECK(TestMem::live == 0);
  owners();
  CHECK(TestMem::live == 0); // every destructor has run: nothing is left
  CHECK(fail_at == 0 || TestMem::calls >= fail_at);
  return TestMem::calls;
}

} // namespace

int main()
{
  const long n = scenario(0);
  CHECK(n == 3 + 1 + 10 + 2); // single: first allocation, growth, renewal, the 16-byte floor; group: 2 x 5; owners: 2
  for (long k = 1; k <= n; ++k) scenario(k);
  CHECK(TestMem::live == 0);
  printf("buf_check: ok (%ld allocations, each failed once)\n", n);
  return 0;
}
