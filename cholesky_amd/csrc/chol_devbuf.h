// Owning device buffers of the C ABI glue (the chol_api*.cpp files only, through chol_device.h).  A dev_buf<T> holds one device allocation of the library's own: it starts empty, is
// move-only and releases what it holds when it goes out of scope or takes something else.  Whatever can fail returns the library's error code with
// the error text set and leaves the buffer EMPTY: "non-empty" always means "allocated and initialised as asked".  No HIP here: memory comes and goes
// through the four functions below, which chol_api.cpp defines over the HIP runtime and tests/native/devbuf_host.cpp over malloc.
#ifndef CHOL_DEVBUF_H
#define CHOL_DEVBUF_H
#include <cstddef>
#include <type_traits>

// floating_point: scratch of a floating-point type (poisoned and guarded under CHOLAMD_POISON); 0: exactly `bytes` of plain device memory.  *p is
// NULL after a failure.  The release is synchronous.  Both keep the count behind cholamd_debug_live_buffers().
int chol_dev_acquire(void **p, size_t bytes, int floating_point);
void chol_dev_release(void *p);
int chol_dev_zero(void *p, size_t bytes);
int chol_dev_copy_in(void *p, const void *host, size_t bytes);

template <class T> class dev_buf { // dev_buf<char>: a byte buffer, and what a container of buffers of several types holds
  void *p_ = nullptr;
public:
  dev_buf() = default;
  dev_buf(const dev_buf &) = delete;
  dev_buf &operator=(const dev_buf &) = delete;
  dev_buf(dev_buf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  dev_buf &operator=(dev_buf &&o) noexcept { if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; } return *this; }
  ~dev_buf() { reset(); }
  void reset() { if (p_) chol_dev_release(p_); p_ = nullptr; }
  T *get() const { return static_cast<T *>(p_); }
  operator T *() const { return get(); } // launch arguments, pointer arithmetic
  explicit operator bool() const { return p_ != nullptr; }
  // alloc*, upload*: replace what the buffer holds.  upload*: a plain allocation of the exact size, filled from the host; no elements: empty
  int alloc_bytes(size_t bytes, int floating_point = std::is_floating_point<T>::value) { reset(); return chol_dev_acquire(&p_, bytes, floating_point); }
  int alloc(size_t n) { return alloc_bytes(n * sizeof(T)); }
  int alloc_zero(size_t n) { int rc = alloc(n); if (!rc && (rc = chol_dev_zero(p_, n * sizeof(T)))) reset(); return rc; }
  int upload_bytes(const void *host, size_t bytes) { int rc = alloc_bytes(bytes, 0); if (!rc && (rc = chol_dev_copy_in(p_, host, bytes))) reset(); return rc; }
  int upload(const T *host, size_t n) { reset(); return n ? upload_bytes(host, n * sizeof(T)) : 0; }
  int ensure(size_t n) { return p_ ? 0 : alloc(n); } // allocate at first use
  int ensure_zero(size_t n) { return p_ ? 0 : alloc_zero(n); }
};
#endif
