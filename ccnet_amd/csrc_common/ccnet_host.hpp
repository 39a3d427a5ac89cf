// ccnet_host.hpp -- the host-side prologue that the x_api.hip of the OHEM, evaluation, Lovász and ABN libraries share: the
// error text behind ccnet_x_last_error_string(), workspace carving, the launch check.  The including translation unit defines
// CCNET_ERROR_PREFIX ("ccnet_x: ") first and includes this header after its x_kernels.hpp, which brings the HIP runtime (in the
// CPU test-suite: the emulator's stand-in) through <x_platform.hpp>.  Everything sits in an unnamed namespace and each library
// is one translation unit, so the error buffers stay one per library and per thread.
#pragma once
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>

#ifndef CCNET_ERROR_PREFIX
#error "define CCNET_ERROR_PREFIX (\"ccnet_x: \") before including ccnet_host.hpp"
#endif

namespace {

thread_local char g_err[256] = "";

inline int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    int n = snprintf(g_err, sizeof g_err, CCNET_ERROR_PREFIX);
    vsnprintf(g_err + n, sizeof g_err - n, fmt, ap);
    va_end(ap);
    return code;
}

inline size_t align256(size_t n) { return (n + 255) & ~size_t(255); }

template <class T>
T *at(void *ws, size_t off) { return reinterpret_cast<T *>(static_cast<char *>(ws) + off); }

inline int launched(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-4, "%s launch failed: %s", what, hipGetErrorString(e));
    return 0;
}

}  // namespace
