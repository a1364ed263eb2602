// lstm_device.h — device helpers shared by the three recurrence kernels (lstm.hip, lstm_persist.hip, lstm_wide.hip).
// The recurrence kinds must produce the same bits (re-arming switches kinds in the middle of a run), so their cell
// math exists once, here.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace nasr {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) unsigned gu32;
typedef volatile __attribute__((address_space(3))) unsigned lds_vu32;   // a volatile access through a GENERIC pointer to LDS
                                                                        // compiles to flat_store sc0 sc1 + vmcnt(0)

// The bare v_exp_f32 (2^x), without the denormal scaling __expf can wrap around it: an exponential that overflows to inf
// or flushes to 0 gives the saturated value of the sigmoid / tanh either way, and in the normal range the two are the
// same instruction on the same input (results bitwise equal; measured time equal too - the cell wave's chain is latency,
// not issue).
__device__ __forceinline__ float exp_(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }
__device__ __forceinline__ float sigmoidf_(float x) { return __builtin_amdgcn_rcpf(1.f + exp_(-x)); }
__device__ __forceinline__ float tanhf_(float x) { return 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + exp_(2.f * x)); }

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

constexpr unsigned SPIN_BUDGET = 1u << 21;   // polls before a wave gives up (~0.5 s)

// wait until every active lane's word is >= want (monotonic step counters; wrap-safe compare)
__device__ __forceinline__ bool poll_ge(gu32* p, bool active, unsigned want) {
  for (unsigned n = 0; n < SPIN_BUDGET; ++n) {
    const unsigned v = active ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : want;
    if (__all((int)(v - want) >= 0)) return true;
  }
  return false;
}

}  // namespace nasr
