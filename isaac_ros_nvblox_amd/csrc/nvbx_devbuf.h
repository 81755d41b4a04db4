// nvbx_devbuf.h -- how the mapper's device memory is owned (host code only): the scratch buffers that grow on demand (DevBuf) and
// the entry type of the one table that names the map's device arrays (PoolArr; the table is nvbx_mapper::pool_arrays, mapper.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "../../include/nvblox_hip.h"

namespace nvbx {
void set_error(const char* what, hipError_t e);

// Device memory that grows on demand and never shrinks; the contents are NOT kept across a growth.
struct DevBuf {
  void* p = nullptr; size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; } return *this; }
  ~DevBuf() { release(); }
  // at least `need` bytes.  Enough already: a compare and a return (the per-frame path: no call into HIP).  Else the launches on `s` that
  // may still use the old memory finish first; on failure the buffer is empty.  *grew = true only where the memory was replaced.
  int ensure(hipStream_t s, size_t need, bool* grew = nullptr) { return need <= bytes ? NVBX_OK : grow(s, need, grew); }
  void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }      // (the caller has made the streams that use it idle)
  template <typename T> T* as() const { return static_cast<T*>(p); }

 private:
  int grow(hipStream_t s, size_t need, bool* grew) {
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) { set_error("DevBuf: hipStreamSynchronize", e); return NVBX_E_DEVICE; }
    if (p) { e = hipFree(p); if (e != hipSuccess) { set_error("DevBuf: hipFree", e); return NVBX_E_DEVICE; } }
    p = nullptr; bytes = 0;
    e = hipMalloc(&p, need);
    if (e != hipSuccess) { p = nullptr; set_error("DevBuf: hipMalloc", e); return NVBX_E_DEVICE; }
    bytes = need;
    if (grew) *grew = true;
    return NVBX_OK;
  }
};

// One device array of the map, by the address of the pointer the kernels take by value.  `bytes`: its size at the capacity the table was made
// for; 0 = allocated on first use by code of its own (null until then).  bytes_per_block > 0: one record of that size per block -- pool growth
// re-allocates it, copies it and fills the new tail with `fill` (-1: left as it is); 0: regrown by special code of grow_map, or never.
struct PoolArr { void** p; size_t bytes_per_block; int fill; size_t bytes; };

}  // namespace nvbx
