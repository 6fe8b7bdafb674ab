// Host side of a library that is built from one source of its own (wavenet_amd/build.py: SIDE_LIBS): the text of the last
// error, the refusal of an argument, the dynamic-LDS limit of a kernel and the status of a launch.  Host code only.
//
// The source defines WN_SIDE_EARG and WN_SIDE_EHIP as its library's own codes (WNL_EARG, WNL_EHIP, ...) before it includes this
// header.  Everything sits in an anonymous namespace: each library has its own buffer and the libraries share no symbol.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

namespace wn {
namespace {

thread_local char g_err[512] = "";
int fail(int rc, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return rc;
}
#define WN_CHECK_ARG(cond, ...)                              \
    do {                                                     \
        if (!(cond)) return fail(WN_SIDE_EARG, __VA_ARGS__); \
    } while (0)

// A launch may ask for 48 KB of dynamic LDS without more ado; above that the kernel's limit is raised first.  The attribute
// belongs to the device that is current, so it is set by the call that needs it (a host-side call, nothing is enqueued),
// not once per process: another device, or a call after a failed one, is served like the first.  0, or WN_SIDE_EHIP.
template <typename Kernel>
int raise_lds_limit(Kernel kernel, const char* name, long long lds_bytes) {
    if (lds_bytes <= 48 * 1024) return 0;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)lds_bytes);
    if (e == hipSuccess) return 0;
    return fail(WN_SIDE_EHIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize, %lld) failed for %s: %s", lds_bytes, name,
                hipGetErrorString(e));
}

// after hipLaunchKernelGGL: 0 (every library's *_OK), or WN_SIDE_EHIP with the launch's error under the entry point's name
int launch_status(const char* entry) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail(WN_SIDE_EHIP, "%s: kernel launch failed: %s", entry, hipGetErrorString(e));
}

}  // namespace
}  // namespace wn
