// v2v_status.hpp -- how every C entry point of libv2v_hip.so reports a failure: one thread-local message behind v2v_last_error()
// (include/v2v_hip.h).  The buffer and these functions are defined once, in v2v_capi.hip; every translation unit that holds entry
// points includes this header.  Host code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace v2v {

// stores the formatted message for the calling thread and returns `code` (so that `return fail(V2V_ERR_..., ...)` is the whole error path)
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// V2V_ERR_HIP with "<what>: <HIP's error string> (<code>)"
int hip_fail(hipError_t e, const char *what);

// after a launch: V2V_OK, or hip_fail(hipGetLastError(), what)
int launched(const char *what);

inline bool aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

}  // namespace v2v
