// The timing experiments and phase stamps of the trace library (`make TRACE=1` -> libconvdr_hip_trace.so), device and host.
//
// An experiment knob makes a kernel skip or repeat work to bound what that work costs: its results are garbage by design.  A
// trace pointer receives s_memtime stamps of a kernel's phases.  Neither belongs in the product library, so both live HERE
// and nowhere else: every kernel argument struct that an experiment touches ends in one `TraceKnobs knobs` member, and every
// kernel reads it through the accessors below.
//   CONVDR_ENABLE_TRACE defined: the knobs are data in the argument struct, written by the launchers from the CONVDR_DBG_*
//     environment and the convdr_set_option("gemm_trace" | "gemm_trace_ln" | "attn_trace") pointers, read at run time.
//   product build: the struct is empty and the accessors are constexpr zeros -- every `if (a.knobs.skip_epi() == 1)` folds
//     away at compile time and no experiment path reaches a product kernel.  A host line that writes a knob outside
//     #ifdef CONVDR_ENABLE_TRACE does not compile.
// Which knob means what to which kernel: GemmArgs (gemm_kernel.hpp), GemmLnArgs (gemm_ln.hpp), ScanArgs (ip_scan.hpp); the
// attention argument structs use the trace pointer only.
// NOT here: GemmArgs::clock_probe.  It is a measurement with correct results -- bench.py reads the FFN1 kernel's shader
// clock through it -- and stays an ordinary argument in both builds.
#pragma once
#include <stdlib.h>

#include <type_traits>

namespace convdr {

#ifdef CONVDR_ENABLE_TRACE
struct TraceKnobs {
  int v_same_tile = 0, v_skip_epi = 0, v_prelanded = 0;
  unsigned long long* v_trace = nullptr;
  __host__ __device__ int same_tile() const { return v_same_tile; }
  __host__ __device__ int skip_epi() const { return v_skip_epi; }
  __host__ __device__ int prelanded() const { return v_prelanded; }
  __host__ __device__ unsigned long long* trace() const { return v_trace; }
};
// an integer knob of the environment (0 when unset); the launchers keep the value in a function-local static
inline int env_knob(const char* name) {
  const char* v = getenv(name);
  return v ? atoi(v) : 0;
}
// Host-only knobs of the training step (train.hip says which bit drops or doubles which class of launches)
inline int skip_classes() { static const int v = env_knob("CONVDR_DBG_SKIP"); return v; }
inline int double_classes() { static const int v = env_knob("CONVDR_DBG_DOUBLE"); return v; }
#else
struct TraceKnobs {
  static constexpr int same_tile() { return 0; }
  static constexpr int skip_epi() { return 0; }
  static constexpr int prelanded() { return 0; }
  static constexpr unsigned long long* trace() { return nullptr; }
};
static_assert(std::is_empty<TraceKnobs>::value, "the product build carries no experiment data into a kernel");
constexpr int skip_classes() { return 0; }
constexpr int double_classes() { return 0; }
#endif

}  // namespace convdr
