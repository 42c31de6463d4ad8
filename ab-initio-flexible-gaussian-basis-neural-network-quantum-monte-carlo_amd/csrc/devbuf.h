// devbuf.h -- DevBuf, the one owner of device memory on the host side: a device pointer and its
// capacity in bytes, grow-only, freed by its destructor.  Every device buffer of aiqmc_ctx is one.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
  ~DevBuf() { release(); }

  // at least `bytes` of capacity: nothing when it is there already, else free, then hipMalloc
  // (the contents are not kept); *grew (optional) says whether the buffer was reallocated
  hipError_t reserve(size_t bytes, bool* grew = nullptr) {
    if (grew) *grew = bytes > cap_;
    if (bytes <= cap_) return hipSuccess;
    release();
    const hipError_t e = hipMalloc(&p_, bytes);
    if (e == hipSuccess) cap_ = bytes;
    else p_ = nullptr;
    return e;
  }
  void release() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr, cap_ = 0;
  }
  size_t capacity() const { return cap_; }
  explicit operator bool() const { return p_ != nullptr; }
  template <typename T = void>
  T* as() const { return static_cast<T*>(p_); }

 private:
  void* p_ = nullptr;
  size_t cap_ = 0;
};
