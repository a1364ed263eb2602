// optim.hip — fused TF-flavoured Adam over the flat parameter buffer and the small deterministic
// reductions (bias column sums, slab sums).
//
// tf.train.AdamOptimizer (networks/tfnetwork.py:116-117,139):
//   lr_t = lr*sqrt(1-b2^t)/(1-b1^t) (t counted and lr_t computed on the device);  m <- b1 m + (1-b1) g;  v <- b2 v + (1-b2) g^2;
//   p <- p - lr_t * m / (sqrt(v) + eps)          (eps NOT bias-corrected)
// `gscale` folds average_gradients' 1/num_towers (networks/tfnetwork.py:72-86) into the same pass.
// One pass reads g,m,v,p and writes m,v,p with 16-byte accesses: 28 B/param, HBM-bound.
//
// Global-norm gradient clipping with a non-finite guard (nasr_set_grad_clip; the reference has neither): a deterministic
// two-stage fp64 sum of squares of the gradient buffer, whose second stage decides the step on the device and leaves the
// multiplier for the Adam pass in device memory (ClipDev).  With clipping off none of it is launched.
//
// Parameter averaging (nasr_set_ema; the reference has none): tf.train.ExponentialMovingAverage(decay, num_updates) of the
// parameters, E <- E + (1 - d_n)(P_new - E) with d_n = min(decay, (1 + n) / (10 + n)), inside the same sweep on the p the
// Adam line has just produced: 36 B/param.  n and 1 - d_n live on the device (EmaDev) and advance where Adam's count does,
// so a void or skipped step leaves the average alone.  With averaging off the sweeps launched are the two above, unchanged.
#include "kernels.h"

#include <cstdlib>

namespace nasr {

const char* test_hook(const char* name) {
  static const bool enabled = [] {
    const char* e = getenv("NASR_TEST_HOOKS");
    return e && e[0] == '1';
  }();
  return enabled ? getenv(name) : nullptr;
}

// t <- t + 1 and lr_t = lr*sqrt(1-b2^t)/(1-b1^t) in double, by one thread
__device__ __forceinline__ void adam_advance(AdamDev* st, float lr, float b1, float b2) {
  const long long t = st->step + 1;
  st->step = t;
  st->lr_t = (float)((double)lr * sqrt(1.0 - pow((double)b2, (double)t)) / (1.0 - pow((double)b1, (double)t)));
  st->applied = 1;
}

// n <- n + 1 and omd = 1 - min(decay, (1 + n) / (10 + n)) in double, by the same thread (em NULL: no averaging)
__device__ __forceinline__ void ema_advance(EmaDev* em, float decay) {
  if (!em) return;
  const long long n = em->updates;
  const double ramp = (1.0 + (double)n) / (10.0 + (double)n);
  const double d = (double)decay < ramp ? (double)decay : ramp;
  em->omd = (float)(1.0 - d);
  em->updates = n + 1;
}

// ... unless the step is void
__global__ void adam_prepare_kernel(AdamDev* st, const float* __restrict__ fault, float lr, float b1, float b2, EmaDev* em,
                                    float decay) {
  if (fault && *fault != 0.f) {
    st->applied = 0;
    return;
  }
  adam_advance(st, lr, b1, b2);
  ema_advance(em, decay);
}

// the sweep of the Adam kernels, behind their void-step check; `gscale` is the step's multiplier and `lr_t` its step size.
// EMA (a literal): the average e follows the new p in the same trip, e <- fma(omd, p - e, e).
#define NASR_ADAM_SWEEP(EMA)                                                                                              \
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {       \
    float4 gg = reinterpret_cast<const float4*>(g)[i];                                                                    \
    float4 mm = reinterpret_cast<float4*>(m)[i];                                                                          \
    float4 vv = reinterpret_cast<float4*>(v)[i];                                                                          \
    float4 pp = reinterpret_cast<float4*>(p)[i];                                                                          \
    NASR_ADAM1(x) NASR_ADAM1(y) NASR_ADAM1(z) NASR_ADAM1(w)                                                               \
    reinterpret_cast<float4*>(m)[i] = mm;                                                                                 \
    reinterpret_cast<float4*>(v)[i] = vv;                                                                                 \
    reinterpret_cast<float4*>(p)[i] = pp;                                                                                 \
    NASR_EMA_##EMA                                                                                                        \
  }
#define NASR_EMA_0
#define NASR_EMA_1                                                                                                        \
  {                                                                                                                       \
    float4 ee = reinterpret_cast<float4*>(e)[i];                                                                          \
    ee.x = fmaf(omd, pp.x - ee.x, ee.x);                                                                                  \
    ee.y = fmaf(omd, pp.y - ee.y, ee.y);                                                                                  \
    ee.z = fmaf(omd, pp.z - ee.z, ee.z);                                                                                  \
    ee.w = fmaf(omd, pp.w - ee.w, ee.w);                                                                                  \
    reinterpret_cast<float4*>(e)[i] = ee;                                                                                 \
  }
#define NASR_ADAM1(c)                                   \
  {                                                     \
    const float gc = gg.c * gscale;                     \
    mm.c = b1 * mm.c + (1.f - b1) * gc;                 \
    vv.c = b2 * vv.c + (1.f - b2) * gc * gc;            \
    pp.c = pp.c - lr_t * mm.c / (sqrtf(vv.c) + eps);    \
  }

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                   const float* __restrict__ g, int64_t n4, const AdamDev* __restrict__ st,
                                                   float b1, float b2, float eps, float gscale,
                                                   const float* __restrict__ fault) {
  // A persistent-recurrence launch that gave up marks the gradient buffer's fault word (it is all-reduced with the
  // gradients, so every rank sees it): such a step must not touch the parameters, on any rank.
  if (fault && *fault != 0.f) return;
  const float lr_t = st->lr_t;
  NASR_ADAM_SWEEP(0)
}

// the same with the average e behind p; omd = 1 - d_n of this step (ema_advance)
__global__ __launch_bounds__(256) void adam_ema_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                       const float* __restrict__ g, float* __restrict__ e, int64_t n4,
                                                       const AdamDev* __restrict__ st, const EmaDev* __restrict__ em, float b1,
                                                       float b2, float eps, float gscale, const float* __restrict__ fault) {
  if (fault && *fault != 0.f) return;
  const float lr_t = st->lr_t;
  const float omd = em->omd;
  NASR_ADAM_SWEEP(1)
}

// the same with the multiplier of this step read from ClipDev: grad_scale * coef, or nothing at all for a skipped step
__global__ __launch_bounds__(256) void adam_clip_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                        const float* __restrict__ g, int64_t n4,
                                                        const AdamDev* __restrict__ st, const ClipDev* __restrict__ clip,
                                                        float b1, float b2, float eps, const float* __restrict__ fault) {
  if (fault && *fault != 0.f) return;
  if (clip->skip) return;
  const float lr_t = st->lr_t;
  const float gscale = clip->s;
  NASR_ADAM_SWEEP(0)
}

__global__ __launch_bounds__(256) void adam_clip_ema_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                            const float* __restrict__ g, float* __restrict__ e, int64_t n4,
                                                            const AdamDev* __restrict__ st, const ClipDev* __restrict__ clip,
                                                            const EmaDev* __restrict__ em, float b1, float b2, float eps,
                                                            const float* __restrict__ fault) {
  if (fault && *fault != 0.f) return;
  if (clip->skip) return;
  const float lr_t = st->lr_t;
  const float gscale = clip->s;
  const float omd = em->omd;
  NASR_ADAM_SWEEP(1)
}
#undef NASR_ADAM1
#undef NASR_EMA_0
#undef NASR_EMA_1
#undef NASR_ADAM_SWEEP

// a <-> b over n4 float4s (nasr_ema_swap: the data move, the pointers and every offset into them stay)
__global__ __launch_bounds__(256) void swap16_kernel(float4* __restrict__ a, float4* __restrict__ b, int64_t n4) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 x = a[i], y = b[i];
    a[i] = y;
    b[i] = x;
  }
}

// ---- the global norm: n2 = sum_i (double)g_i * (double)g_i, the same bits on every run ----------------------------------
// The square of an fp32 value is exact in fp64 and every partial sum is rounded once, in an order that depends on the
// element count alone: lane j of workgroup b adds the float4s lo_b + j, lo_b + j + 256, ... of b's contiguous share
// (one accumulator per component, combined (x+y)+(z+w)), the 64 lanes of a wave fold by halves (32, 16, ... 1), the four
// waves combine through LDS as (0+1)+(2+3).  No atomics.
__device__ __forceinline__ double block_sum_fixed(double a, double* sm) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = a;
  __syncthreads();
  return (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

int grad_sumsq_blocks(int64_t n) {
  const int64_t b = (n / 4 + 255) / 256;    // a share is at least one 16-byte load per lane
  return b < 1 ? 1 : b > GRAD_SUMSQ_MAX_BLOCKS ? GRAD_SUMSQ_MAX_BLOCKS : (int)b;
}

__global__ __launch_bounds__(256) void grad_sumsq_part_kernel(const float* __restrict__ g, int64_t n,
                                                              double* __restrict__ part, const float* __restrict__ fault) {
  __shared__ double sm[4];
  if (fault && *fault != 0.f) return;   // a void step: nothing is measured (grad_clip_final_kernel returns as well)
  const int64_t n4 = n / 4;
  const int64_t per = (n4 + gridDim.x - 1) / gridDim.x;
  const int64_t lo = per * blockIdx.x, hi = lo + per < n4 ? lo + per : n4;
  double ax = 0.0, ay = 0.0, az = 0.0, aw = 0.0;
#pragma unroll 4
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
    const float4 v = reinterpret_cast<const float4*>(g)[i];
    ax += (double)v.x * (double)v.x;
    ay += (double)v.y * (double)v.y;
    az += (double)v.z * (double)v.z;
    aw += (double)v.w * (double)v.w;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int64_t i = n4 * 4; i < n; ++i) ax += (double)g[i] * (double)g[i];   // (every layout here is a multiple of 4)
  const double s = block_sum_fixed((ax + ay) + (az + aw), sm);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// One workgroup: thread j adds the partials j, j + 256, ... in index order, then the same fixed fold; thread 0 decides the
// step.  A void step (fault word set) leaves everything alone, as adam_prepare_kernel does, whose work this kernel takes
// over: a step that is applied advances Adam's count (and the average's), a skipped one (non-finite norm) does not.
__global__ __launch_bounds__(256) void grad_clip_final_kernel(const double* __restrict__ part, int nparts, ClipDev* clip,
                                                              AdamDev* st, const float* __restrict__ fault, float gscale,
                                                              float max_norm, float lr, float b1, float b2, EmaDev* em,
                                                              float decay) {
  __shared__ double sm[4];
  if (fault && *fault != 0.f) {
    if (threadIdx.x == 0) st->applied = 0;
    return;
  }
  double a = 0.0;
  for (int k = threadIdx.x; k < nparts; k += 256) a += part[k];
  const double n2 = block_sum_fixed(a, sm);
  if (threadIdx.x != 0) return;
  const double norm = fabs((double)gscale) * sqrt(n2);
  clip->last_norm = norm;
  if (!isfinite(norm)) {            // an inf or a NaN somewhere in the gradient: P, M, V and t stay as they are
    clip->skip = 1;
    clip->skipped += 1;
    st->applied = 0;
    return;
  }
  const float coef = (float)(norm > (double)max_norm ? (double)max_norm / norm : 1.0);   // tf.clip_by_global_norm
  clip->skip = 0;
  clip->s = gscale * coef;          // == gscale exactly when coef == 1
  clip->last_coef = coef;
  clip->steps += 1;
  if (coef < 1.f) clip->clipped += 1;
  if (norm > clip->window_max_norm) clip->window_max_norm = norm;
  adam_advance(st, lr, b1, b2);
  ema_advance(em, decay);
}

void launch_adam(float* p, float* m, float* v, const float* g, int64_t n, AdamDev* state, float lr, float beta1, float beta2,
                 float eps, float gscale, const float* fault, float* e, EmaDev* ema, float decay, hipStream_t st) {
  const int64_t n4 = n / 4;
  int blocks = (int)((n4 + 255) / 256);
  if (blocks > ADAM_MAX_BLOCKS) blocks = ADAM_MAX_BLOCKS;
  hipLaunchKernelGGL(adam_prepare_kernel, dim3(1), dim3(1), 0, st, state, fault, lr, beta1, beta2, e ? ema : nullptr, decay);
  if (e)
    hipLaunchKernelGGL(adam_ema_kernel, dim3(blocks), dim3(256), 0, st, p, m, v, g, e, n4, state, ema, beta1, beta2, eps, gscale,
                       fault);
  else
    hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(256), 0, st, p, m, v, g, n4, state, beta1, beta2, eps, gscale, fault);
}

void launch_swap16(float* a, float* b, int64_t n, hipStream_t st) {
  const int64_t n4 = n / 4;
  int blocks = (int)((n4 + 255) / 256);
  if (blocks > ADAM_MAX_BLOCKS) blocks = ADAM_MAX_BLOCKS;
  hipLaunchKernelGGL(swap16_kernel, dim3(blocks), dim3(256), 0, st, reinterpret_cast<float4*>(a), reinterpret_cast<float4*>(b), n4);
}

void launch_adam_clipped(float* p, float* m, float* v, const float* g, int64_t n, AdamDev* state, ClipDev* clip, double* part,
                         float lr, float beta1, float beta2, float eps, float gscale, float max_norm, const float* fault,
                         float* e, EmaDev* ema, float decay, hipStream_t st) {
  const int64_t n4 = n / 4;
  int blocks = (int)((n4 + 255) / 256);
  if (blocks > ADAM_MAX_BLOCKS) blocks = ADAM_MAX_BLOCKS;
  const int nparts = grad_sumsq_blocks(n);
  hipLaunchKernelGGL(grad_sumsq_part_kernel, dim3(nparts), dim3(256), 0, st, g, n, part, fault);
  hipLaunchKernelGGL(grad_clip_final_kernel, dim3(1), dim3(256), 0, st, part, nparts, clip, state, fault, gscale, max_norm, lr,
                     beta1, beta2, e ? ema : nullptr, decay);
  if (e)
    hipLaunchKernelGGL(adam_clip_ema_kernel, dim3(blocks), dim3(256), 0, st, p, m, v, g, e, n4, state, clip, ema, beta1, beta2,
                       eps, fault);
  else
    hipLaunchKernelGGL(adam_clip_kernel, dim3(blocks), dim3(256), 0, st, p, m, v, g, n4, state, clip, beta1, beta2, eps, fault);
}

// ---- column sums: stage 1 writes part[rs][n] for 32 row slices, stage 2 adds them in order
constexpr int CS_SPLIT = 32;

__global__ __launch_bounds__(256) void colsum_part_kernel(const float* __restrict__ M, int R, int N, int ld,
                                                          float* __restrict__ part) {
  __shared__ float sm[4][64];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int n = blockIdx.x * 64 + cx;
  const int rs = blockIdx.y;
  const int per = (R + CS_SPLIT - 1) / CS_SPLIT;
  const int r0 = rs * per, r1 = min(R, r0 + per);
  float s = 0.f;
  if (n < N)
    for (int r = r0 + ry; r < r1; r += 4) s += M[(size_t)r * ld + n];
  sm[ry][cx] = s;
  __syncthreads();
  if (ry == 0 && n < N) part[(size_t)rs * N + n] = (sm[0][cx] + sm[1][cx]) + (sm[2][cx] + sm[3][cx]);
}

// fixed-order sum of `nparts` partial rows: 16 columns per block, 16 threads per column (rows q, q+16, ...) combined
// through LDS in a fixed order - 4x the blocks and a quarter of the dependent loads of the 64-column form (12.9 -> ~5 us
// for 125 x 4096)
__global__ __launch_bounds__(256) void colsum_final_kernel(const float* __restrict__ part, int nparts, int N,
                                                           float* __restrict__ out) {
  __shared__ float sm[16][17];
  const int cx = threadIdx.x & 15, q = threadIdx.x >> 4;
  const int n = blockIdx.x * 16 + cx;
  float s = 0.f;
  if (n < N)
    for (int k = q; k < nparts; k += 16) s += part[(size_t)k * N + n];
  sm[q][cx] = s;
  __syncthreads();
  if (q == 0 && n < N) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += sm[i][cx];
    out[n] = t;
  }
}

void launch_colsum_parts(const float* part, int nparts, int N, float* out, hipStream_t st) {
  hipLaunchKernelGGL(colsum_final_kernel, dim3((N + 15) / 16), dim3(256), 0, st, part, nparts, N, out);
}

void launch_colsum(const float* M, int R, int N, int ld, float* out, float* ws, hipStream_t st) {
  hipLaunchKernelGGL(colsum_part_kernel, dim3((N + 63) / 64, CS_SPLIT), dim3(256), 0, st, M, R, N, ld, ws);
  launch_colsum_parts(ws, CS_SPLIT, N, out, st);
}

__global__ __launch_bounds__(256) void reduce_slabs_kernel(const float* __restrict__ slabs, int S, int64_t n,
                                                           float* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float s = slabs[i];
    for (int k = 1; k < S; ++k) s += slabs[(size_t)k * n + i];
    out[i] = s;
  }
}
void launch_reduce_slabs(const float* slabs, int S, int64_t n, float* out, hipStream_t st) {
  int blocks = (int)((n + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(reduce_slabs_kernel, dim3(blocks), dim3(256), 0, st, slabs, S, n, out);
}

// the same for a result whose rows are scattered: out[map[m] * ldc + n] = sum_s slabs[s][m][n] (rows with map[m] < 0 dropped)
__global__ __launch_bounds__(256) void reduce_slabs_rows_kernel(const float* __restrict__ slabs, int S, int M, int N, int ldc,
                                                                const int* __restrict__ map, float* __restrict__ out) {
  const int64_t n4 = (int64_t)M * N / 4, per = (int64_t)M * N;
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const int m = (int)(i * 4 / N), c = (int)(i * 4 % N);
    const int orow = map[m];
    if (orow < 0) continue;
    float4 a = *reinterpret_cast<const float4*>(slabs + i * 4);
    for (int s = 1; s < S; ++s) {
      const float4 b = *reinterpret_cast<const float4*>(slabs + s * per + i * 4);
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    *reinterpret_cast<float4*>(out + (size_t)orow * ldc + c) = a;
  }
}
void launch_reduce_slabs_rows(const float* slabs, int S, int M, int N, int ldc, const int* map, float* out, hipStream_t st) {
  int blocks = (int)(((int64_t)M * N / 4 + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(reduce_slabs_rows_kernel, dim3(blocks), dim3(256), 0, st, slabs, S, M, N, ldc, map, out);
}

// ---- diagnostics: a kernel shaped like a ring all-reduce step ---------------------------------------------------------
// `nblocks` workgroups of 256 threads; each sweeps its slice of the buffer `passes` times with 16-byte loads and stores
// (x * 1: the data keep their bits), i.e. it holds its CUs for as long as RCCL's ring kernels hold theirs and moves bytes
// the way they do - what a single GPU can show of a collective that co-runs with the step (nasr_diag_bucket_traffic).
__global__ __launch_bounds__(256) void ring_standin_kernel(float4* __restrict__ buf, long long n4, int passes) {
  const long long per = (n4 + gridDim.x - 1) / gridDim.x;
  const long long lo = per * blockIdx.x, hi = lo + per < n4 ? lo + per : n4;
  for (int p = 0; p < passes; ++p)
    for (long long i = lo + threadIdx.x; i < hi; i += 256) {
      float4 v = buf[i];
      v.x *= 1.f; v.y *= 1.f; v.z *= 1.f; v.w *= 1.f;
      asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));    // keep the multiply and the store
      buf[i] = v;
    }
}

void launch_ring_standin(float* buf, int64_t n, int nblocks, int passes, hipStream_t st) {
  // buckets start at multiples of 32 floats from a 256-byte aligned allocation: 16-byte accesses are aligned
  hipLaunchKernelGGL(ring_standin_kernel, dim3(nblocks), dim3(256), 0, st, reinterpret_cast<float4*>(buf), (long long)(n / 4), passes);
}

}  // namespace nasr
