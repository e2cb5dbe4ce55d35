// Device scratch of the host layer (densecap.hip): carve lists, a call-scoped owner and a grow-only buffer.  Host code only.
//
// The runtime is touched through three calls -- hipMalloc, hipFree, hipStreamSynchronize -- and the names hipError_t, hipSuccess,
// hipErrorInvalidValue and hipStream_t; a failure comes back as the hipError_t, for the caller's HIPCHK to report (the error
// string is formed there).  A stand-alone host program (tests/scratch_host.cpp) defines DC_SCRATCH_STANDIN and declares
// counting stand-ins of those names before it includes this file.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#ifndef DC_SCRATCH_STANDIN
#include <hip/hip_runtime.h>
#endif

// Pieces of one allocation: `carve(cv, base)` points each *p at its own 256-byte aligned piece of `base` and returns the
// bytes all of them take (base = null: only the bytes).
inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }
struct Carve { void** p; size_t bytes; };
inline size_t carve(const std::vector<Carve>& cv, void* base) {
  size_t total = 0;
  for (const Carve& c : cv) {
    if (base != nullptr) *c.p = static_cast<char*>(base) + total;
    total += al(c.bytes);
  }
  return total;
}

// What a context's scratch owners count (dc_debug_fetch "scratch"): Scratch blocks alive now, bytes the KeptBufs hold, and how
// many times a KeptBuf has been (re)allocated.
struct ScratchStats { int64_t live = 0, kept_bytes = 0, kept_allocs = 0; };

// One device block that lives as long as the call that made it: allocated once, from a byte count or a carve list, freed by the
// destructor after the stream the call enqueued on has drained.  A function that holds one may return from anywhere.
class Scratch {
 public:
  Scratch(ScratchStats& st, hipStream_t s) : st_(st), s_(s) {}
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
  ~Scratch() {
    if (p_ == nullptr) return;
    (void)hipStreamSynchronize(s_);
    (void)hipFree(p_);
    st_.live -= 1;
  }
  hipError_t alloc(size_t bytes) {
    if (p_ != nullptr) return hipErrorInvalidValue;           // once
    const hipError_t e = hipMalloc(&p_, bytes);
    if (e != hipSuccess) { p_ = nullptr; return e; }
    if (p_ != nullptr) st_.live += 1;
    return hipSuccess;
  }
  hipError_t alloc(const std::vector<Carve>& cv) {
    const hipError_t e = alloc(carve(cv, nullptr));
    if (e == hipSuccess) carve(cv, p_);
    return e;
  }
  void* get() const { return p_; }

 private:
  ScratchStats& st_;
  hipStream_t s_;
  void* p_ = nullptr;
};

// A device block a context keeps between calls and that only grows: `grow` keeps it while the request fits, else drains the
// stream that may still read it, frees it and allocates the new size.  Freed by reset() or the destructor (the device is idle).
class KeptBuf {
 public:
  explicit KeptBuf(ScratchStats& st) : st_(st) {}
  KeptBuf(const KeptBuf&) = delete;
  KeptBuf& operator=(const KeptBuf&) = delete;
  ~KeptBuf() { reset(); }
  hipError_t grow(size_t bytes, hipStream_t s) {
    if (p_ != nullptr && bytes <= bytes_) return hipSuccess;
    if (p_ != nullptr) {
      const hipError_t e = hipStreamSynchronize(s);
      if (e != hipSuccess) return e;
      reset();
    }
    const hipError_t e = hipMalloc(&p_, bytes);
    if (e != hipSuccess) { p_ = nullptr; return e; }
    bytes_ = bytes;
    st_.kept_bytes += (int64_t)bytes;
    st_.kept_allocs += 1;
    return hipSuccess;
  }
  void reset() {
    if (p_ != nullptr) (void)hipFree(p_);
    st_.kept_bytes -= (int64_t)bytes_;
    p_ = nullptr;
    bytes_ = 0;
  }
  void* get() const { return p_; }
  size_t bytes() const { return bytes_; }

 private:
  ScratchStats& st_;
  void* p_ = nullptr;
  size_t bytes_ = 0;
};
