// Host-only helpers of the core library's export layer: what stands between an `extern "C"` export and its kernels.  Nothing here is
// device code and nothing depends on the build: bf16_t is the raw 16-bit storage type in both libraries (COUNTR_HALF_FP16, common.hpp).
// (The block count of a grid-stride launch, countr_blocks_for, is in common.hpp: the side libraries use it too.)
#pragma once
#include "common.hpp"
#include <stdlib.h>
#include <utility>
#include "../../include/countr_hip.h"

// f(T{}) with T = bf16_t for COUNTR_BF16 and float for every other code, as the exports always read a dtype code; f is a generic lambda
// that begins `using T = decltype(t);`.  Exports with an out_bf16 / dy_bf16 flag pass `flag ? COUNTR_BF16 : COUNTR_F32`.
// (The deduced return type has the compiler instantiate this, and with it the lambda's kernels, where it is called and not at the end of
// the file: a unit's kernels are emitted in the order its exports name them, whether an export dispatches through here or by hand.)
template <typename F> static inline auto by_dtype(int dtype, F&& f) { return dtype == COUNTR_BF16 ? f(bf16_t{}) : f(float{}); }
// an export's void* argument as the storage type of the launch
template <typename T> static inline const T* ptr(const void* p) { return static_cast<const T*>(p); }
template <typename T> static inline T* ptr(void* p) { return static_cast<T*>(p); }

// kernel<<<grid, block, lds bytes, stream>>>(args...) on the export's void* stream; an int converts to a dim3 {n, 1, 1}
template <typename... P, typename... A>
static inline void launch_lds(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, void* stream, A&&... args) {
  hipLaunchKernelGGL(kernel, grid, block, lds, STREAM(stream), std::forward<A>(args)...);
}
template <typename... P, typename... A> static inline void launch(void (*kernel)(P...), dim3 grid, dim3 block, void* stream, A&&... args) {
  launch_lds(kernel, grid, block, 0, stream, std::forward<A>(args)...);
}

// an experiment switch: the integer in the environment variable, `unset` where it is not set.  Read on every call (tests and A/B runs
// flip switches inside one process; none of them is on a graph-replay path).
static inline int env_int(const char* name, int unset) {
  const char* e = getenv(name);
  return e ? atoi(e) : unset;
}
