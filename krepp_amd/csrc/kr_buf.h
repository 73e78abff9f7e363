// kr_buf.h — one owning type for every buffer that grows on demand: a pointer and the element count it was allocated
// for, together, so that a capacity cannot outlive its block.  Knows nothing of HIP: where the memory comes from is the
// policy `Mem` (static void* alloc(size_t bytes), null on failure; static void free(void*)).  kr_devutil.h has the two
// real ones (DevBuf: device memory, PinBuf: page-locked host memory), tests/buf_check.cpp one over malloc.
//
// A Buf does not remember a device: it is grown and destroyed where hipSetDevice is already in effect.  Contents are never
// kept across growth, and the old block is freed BEFORE the new one is asked for, so growing never holds both.
#ifndef KR_BUF_H
#define KR_BUF_H

#include <cstddef>
#include <utility>

template <class T, class Mem>
class Buf {
 public:
  Buf() = default;
  Buf(Buf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
  Buf& operator=(Buf&& o) noexcept
  {
    Buf(std::move(o)).swap(*this);
    return *this;
  }
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { reset(); }

  T* get() const { return p_; }
  size_t size() const { return n_; } // elements asked for (0: no block)
  size_t bytes() const { return p_ ? block_bytes(n_) : 0; }
  void swap(Buf& o) noexcept { std::swap(p_, o.p_), std::swap(n_, o.n_); }
  void reset()
  {
    if (p_) Mem::free(p_);
    p_ = nullptr, n_ = 0;
  }
  // a new block of exactly max(16, n * sizeof(T)) bytes; false (and an empty buffer) when there is none to be had
  bool renew(size_t n)
  {
    reset();
    p_ = static_cast<T*>(Mem::alloc(block_bytes(n)));
    n_ = p_ ? n : 0;
    return p_ != nullptr;
  }
  // room for n elements: the block in hand if it has it, else a new one
  bool reserve(size_t n) { return n <= n_ || renew(n); }

 private:
  static size_t block_bytes(size_t n) { return n * sizeof(T) > 16 ? n * sizeof(T) : 16; }
  T* p_ = nullptr;
  size_t n_ = 0;
};

// A group of buffers that share one capacity: afterwards every one holds at least n elements, or every one is empty.
template <class... B>
bool reserve_all(size_t n, B&... b)
{
  if ((b.reserve(n) && ...)) return true;
  (b.reset(), ...);
  return false;
}

#endif
