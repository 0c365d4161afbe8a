// The host-side error path of the side libraries (csrc_<tag>/*.hip; not of api.hip): each library keeps the text of its last refusal per
// thread and hands it out through its own countr_<tag>_last_error().  Everything is in an anonymous namespace, so every library that
// includes this has a g_err of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

namespace {

thread_local char g_err[512] = "";

inline int fail(int rc, const char* msg) {
  strncpy(g_err, msg, sizeof(g_err) - 1);
  g_err[sizeof(g_err) - 1] = 0;
  return rc;
}

// fail() with a printf format
__attribute__((format(printf, 2, 3))) inline int failf(int rc, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return rc;
}

inline bool misaligned(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) != 0; }

// behind the last launch of an export: 0, or the refusal that names what the runtime said
inline int launched(const char* who) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : failf(-10, "%s: launch failed: %s", who, hipGetErrorString(e));
}

}  // namespace
