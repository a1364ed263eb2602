// lstm_device.h — what the three recurrence files (lstm.hip, lstm_persist.hip, lstm_wide.hip) share.
// The recurrence kinds must produce the same bits (re-arming switches kinds in the middle of a run), so the LSTM cell exists
// once, here: the activations and the c / h update of the forward pass (lstm_gates, lstm_state) and the gate derivatives
// of BPTT (lstm_cell_bwd); every kernel calls these.  So does the protocol around the cell that the resident kernels have
// in common: placement (join_xcd), abort (raise_error), the epoch rule of the self-validating exchange buffers (use_epoch),
// the two-plane fp16 split (split_f16x2) and the phase stamps of the diagnostic builds (Stamps).  (The launchers' dispatch
// over a compile-time list of template values, dispatch_int / for_each_int, is in dispatch.h: the CTC launchers use it too.)
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "dispatch.h"
#include "kernels.h"

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

// ------------------------------------------------------------------ the cell
__device__ __forceinline__ f32x4 to_f32x4(float4 v) { return (f32x4){v.x, v.y, v.z, v.w}; }
__device__ __forceinline__ float4 to_float4(f32x4 v) { return make_float4(v.x, v.y, v.z, v.w); }

// activations (si, tj, sf, so) of the four summed pre-activations (i, j, f, o) = x W + b + h U
__device__ __forceinline__ f32x4 lstm_gates(f32x4 pre, float forget_bias) {
  f32x4 act;
  act.x = sigmoidf_(pre.x);
  act.y = tanhf_(pre.y);
  act.z = sigmoidf_(pre.z + forget_bias);
  act.w = sigmoidf_(pre.w);
  return act;
}
// c (in: of the step before, out: of this step) and the returned h.  A masked step does not call this (the caller's
// `valid` decides what it keeps and publishes).
__device__ __forceinline__ float lstm_state(f32x4 act, float& c) {
  c = c * act.z + act.x * act.y;
  return tanhf_(c) * act.w;
}
// BPTT of one cell: dG (i, j, f, o) and dc_out, the dc handed to the step before, from the saved activations, this step's
// c, the c the forward step started from (first: the sequence's first step started from 0, c_prev is not looked at), dh
// and the dc handed back by the step after.  A masked step does not call this: its dG and dc_out are 0.
// lstm_cell_bwd_tc takes tc = tanhf_(c) in place of c (nothing else reads c): a caller that has c early - the persistent
// BPTT kernel's memory wave - takes the tanh off the chain of the wave that does the cell.
__device__ __forceinline__ f32x4 lstm_cell_bwd_tc(f32x4 act, float tc, float c_prev, bool first, float dh, float dc_in,
                                                  float& dc_out) {
  const float dct = dc_in + dh * act.w * (1.f - tc * tc);
  f32x4 dg;
  dg.x = dct * act.y * act.x * (1.f - act.x);
  dg.y = dct * act.x * (1.f - act.y * act.y);
  dg.z = dct * (first ? 0.f : c_prev) * act.z * (1.f - act.z);
  dg.w = dh * tc * act.w * (1.f - act.w);
  dc_out = dct * act.z;
  return dg;
}
__device__ __forceinline__ f32x4 lstm_cell_bwd(f32x4 act, float c, float c_prev, bool first, float dh, float dc_in,
                                               float& dc_out) {
  return lstm_cell_bwd_tc(act, tanhf_(c), c_prev, first, dh, dc_in, dc_out);
}

// v as two fp16 planes: h1 = fp16(v), h2 = fp16(v - h1)
__device__ __forceinline__ void split_f16x2(float v, _Float16& h1, _Float16& h2) {
  h1 = (_Float16)v;
  h2 = (_Float16)(v - (float)h1);
}

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// ------------------------------------------------------------------ hand-off protocol of the resident kernels
constexpr unsigned SPIN_BUDGET = 1u << 21;   // polls before a wave gives up (~0.5 s)

// wait until every active lane's word is >= want (monotonic step counters; wrap-safe compare)
__device__ __forceinline__ bool poll_ge(gu32* p, bool active, unsigned want) {
  for (unsigned n = 0; n < SPIN_BUDGET; ++n) {
    const unsigned v = active ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : want;
    if (__all((int)(v - want) >= 0)) return true;
  }
  return false;
}

// Epoch (0 / 1) of the use of exchange buffer (step & 1) that `step` of `round` is, in a launch of T steps per round: the
// uses of a buffer alternate 1, 0, 1, ... from a cleared buffer.  (A kernel without rounds is round 0.  The buffers are
// CLEARED before every launch: the bit pattern the words carry is then a function of the launch's shape alone, and two
// runs of the same step give the same bits.)
__device__ __forceinline__ unsigned use_epoch(int round, int T, int step) {
  return (unsigned)(round * ((T + 1 - (step & 1)) >> 1) + (step >> 1) + 1) & 1u;
}

// abort: code 1 = a bounded spin gave up, 2 = placement, 4 = fp16 range (XcdCtl::error)
__device__ __forceinline__ void raise_error(XcdCtl* ctl, unsigned* sticky, float* fault, unsigned code) {
  atomicOr(&ctl->error, code);
  if (fault) *fault = 1.f;   // sits behind the gradients: all-reduced with them, makes Adam a no-op on every rank
  // host-visible, never cleared by a launch; the FIRST cause stays (the timeouts it triggers in the other workgroups come
  // half a second later)
  if (sticky && __hip_atomic_load(sticky, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0)
    __hip_atomic_store(sticky, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Placement: xcc = this workgroup's XCD (HW_REG_XCC_ID), member = its ticket within that XCD; nothing is assumed about
// dispatch order.  Goes through info[0..1] (LDS) and clears the nclear words behind them; contains a barrier.  false (and
// error 2 raised) when the placement is not 32 workgroups on each of 8 XCDs: the caller returns.
__device__ __forceinline__ bool join_xcd(XcdCtl* ctl, unsigned* sticky, float* fault, unsigned* info, int nclear,
                                         unsigned& xcc, unsigned& member) {
  if (threadIdx.x == 0) {
    const unsigned x = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 15u;   // HW_REG_XCC_ID[3:0]
    info[0] = x;
    info[1] = x < 8 ? atomicAdd(&ctl->xcc_count[x], 1u) : 0xffffu;
    for (int i = 0; i < nclear; ++i) info[2 + i] = 0;
  }
  __syncthreads();
  xcc = info[0];
  member = info[1];
  if (xcc >= 8 || member >= 32) {
    if (threadIdx.x == 0) raise_error(ctl, sticky, fault, 2u);
    return false;
  }
  return true;
}

// Phase stamps of the diagnostic builds: an enabled wave accumulates the s_memtime ticks between consecutive marks per
// phase and writes its N sums out at the end.  ON = false (every other build) is the empty specialisation below.
template <int N, bool ON>
struct Stamps {
  unsigned long long last;
  unsigned acc[N];
  bool on;
  __device__ __forceinline__ void start(bool enable) {
    on = enable;
    for (int i = 0; i < N; ++i) acc[i] = 0;
    last = __builtin_amdgcn_s_memtime();
  }
  __device__ __forceinline__ void mark(int i) {
    if (on) {
      const unsigned long long t = __builtin_amdgcn_s_memtime();
      acc[i] += (unsigned)(t - last);
      last = t;
    }
  }
  __device__ __forceinline__ void add(int i, unsigned v) {   // a count or an interval taken elsewhere
    if (on) acc[i] += v;
  }
  __device__ __forceinline__ void flush(unsigned* dst) {
    if (on && (threadIdx.x & 63) == 0)
      for (int i = 0; i < N; ++i) dst[i] = acc[i];
  }
};
template <int N>
struct Stamps<N, false> {
  __device__ __forceinline__ void start(bool) {}
  __device__ __forceinline__ void mark(int) {}
  __device__ __forceinline__ void add(int, unsigned) {}
  __device__ __forceinline__ void flush(unsigned*) {}
};

}  // namespace nasr
