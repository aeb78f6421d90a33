// dev_buffers.h -- a handle's device buffers as ONE list that its create, its destroy and whatever allocates later all walk:
// a buffer entered in the list is allocated, zeroed and freed; nothing else has to be kept in step.  And what the entry points
// outside etg_kernels.hip share to refuse a call: fail, hip_fail, device_ptr.  Host code only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include "../../include/etgsim.h"

extern "C" void etg_set_last_error_(const char* msg);

namespace dev {
struct Buf { void** p; size_t bytes; };   // one device buffer of a handle: where its pointer is kept, its size

namespace {   // each translation unit that includes this gets its own copy
int fail(int code, const char* msg) { etg_set_last_error_(msg); return code; }
int fail(int code, const char* who, const char* what) {
  static thread_local char msg[200];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return fail(code, msg);
}
int hip_fail(const char* who, hipError_t e) { return fail(ETG_ERR_HIP, who, hipGetErrorString(e)); }

// Is p device memory?  If so its device becomes the current one: a launch goes to the device that owns the memory, and the
// caller's current device may be another one.  The query alone is no proof -- it can succeed for a host pointer that was never
// registered (type hipMemoryTypeUnregistered) -- so the type is required to be device memory.
bool device_ptr(const void* p) {
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) == hipSuccess && attr.type == hipMemoryTypeDevice &&
      hipSetDevice(attr.device) == hipSuccess) return true;
  (void)hipGetLastError();
  return false;
}

// Allocates the buffers whose pointer is still null (all of them in a value-initialised handle), then zeroes every one: with
// hipMemset, or -- given a stream -- with hipMemsetAsync on it, so that an entry point that takes a stream does not wait.
// On an error the buffers allocated so far stay in their slots, for the handle's destroy to release.
int alloc(const std::vector<Buf>& bufs, const char* who, const hipStream_t* stream = nullptr) {
  for (const Buf& x : bufs) {
    if (!*x.p && hipMalloc(x.p, x.bytes) != hipSuccess) return fail(ETG_ERR_ALLOC, who, "hipMalloc failed");
    if ((stream ? hipMemsetAsync(*x.p, 0, x.bytes, *stream) : hipMemset(*x.p, 0, x.bytes)) != hipSuccess)
      return fail(ETG_ERR_HIP, who, "hipMemset failed");
  }
  return ETG_OK;
}

void release(const std::vector<Buf>& bufs) {
  for (const Buf& x : bufs)
    if (*x.p) (void)hipFree(*x.p);
}
}  // namespace
}  // namespace dev
