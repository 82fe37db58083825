// aqc_dev.hpp — what the HIP translation units of libafterqc_hip.so share on the host side: the error channel behind
// aqc_last_error and the owner of a device allocation.  Internal: nothing here is exported from the library.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "afterqc_hip.h"

namespace aqc {

// Sets the calling thread's aqc_last_error text and returns `code`.  Defined once (aqc_capi.hip, next to the one thread_local
// buffer), so every unit's messages reach aqc_last_error.
__attribute__((visibility("hidden"))) int fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(AQC_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// A device allocation that grows on demand and is freed with its owner.  The owner sees to it that the buffer's device is
// current when it dies (aqc_destroy, ~DeviceInflate), and no DevBuf and no object that owns one — nor one that owns a stream, an
// event or page-locked memory — has static storage, at namespace scope, in a function or inside a container that has: a static
// destructor would call hipFree at exit(), in no fixed order against the HIP runtime's own tear-down and against the statics of
// other units (aqc_host_free's region list).  What is to live as long as the process is held through a plain pointer and never
// deleted: aqc::Keep (aqc_keep.hpp) for objects found by a key, `new` into a `T* const` for a single one (g_compat_buf).
struct __attribute__((visibility("hidden"))) DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    int reserve(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = bytes + bytes / 8 + 256;
        if (hipMalloc(&p, want) != hipSuccess) return -1;
        cap = want;
        return 0;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

}  // namespace aqc
