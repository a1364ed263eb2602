// wavenet.hip — the kernels of the WaveNet CTC network (networks/wavenet.py of the reference) besides its GEMMs, which run
// on gemm.hip's exact-fp32 MFMA kernel: the im2col / col2im of the dilated convolution, batch norm (two-pass per-channel
// statistics, apply, backward), the tanh / gated / residual / skip epilogues and the moving-statistics update.
// Every reduction is a fixed-order sum (per-thread row strides, a tree in LDS, then the row chunks in order): results are
// bitwise reproducible.
#include "wavenet.h"

#include <algorithm>

namespace nasr {

namespace {

constexpr int WN_CH = 32;     // channels per statistics block
constexpr int WN_RG = 8;      // row groups per statistics block (WN_CH * WN_RG threads)

__device__ __forceinline__ float wn_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float wn_rstd(float var, float eps) { return 1.f / sqrtf(var + eps); }

int grid_for(int64_t n, int per = 256) {
  int64_t g = (n + per - 1) / per;
  return (int)(g > 16384 ? 16384 : (g < 1 ? 1 : g));
}

__global__ __launch_bounds__(256) void im2col_kernel(const float* __restrict__ z, float* __restrict__ col, int R, int Bp,
                                                     int D, int KS, int rate) {
  const int D4 = D / 4;
  const int64_t n = (int64_t)R * KS * D4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % D4);
    const int k = (int)((i / D4) % KS);
    const int r = (int)(i / ((int64_t)D4 * KS));
    const int src = r + (k - KS / 2) * rate * Bp;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (src >= 0 && src < R) v = reinterpret_cast<const float4*>(z + (size_t)src * D)[c4];
    reinterpret_cast<float4*>(col + (size_t)r * KS * D + (size_t)k * D)[c4] = v;
  }
}

__global__ __launch_bounds__(256) void col2im_add_kernel(const float* __restrict__ dcol, float* __restrict__ dz, int R,
                                                         int Bp, int D, int KS, int rate) {
  const int D4 = D / 4;
  const int64_t n = (int64_t)R * D4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % D4);
    const int r = (int)(i / D4);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < KS; ++k) {
      const int src = r - (k - KS / 2) * rate * Bp;
      if (src < 0 || src >= R) continue;
      const float4 v = reinterpret_cast<const float4*>(dcol + (size_t)src * KS * D + (size_t)k * D)[c4];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    float4* d = reinterpret_cast<float4*>(dz + (size_t)r * D) + c4;
    float4 o = *d;
    o.x += s.x; o.y += s.y; o.z += s.z; o.w += s.w;
    *d = o;
  }
}

// fixed-order tree over the WN_RG row groups of a block; every thread gets the column's total
__device__ __forceinline__ float block_colsum(float v, float* red) {
  const int c = threadIdx.x % WN_CH, g = threadIdx.x / WN_CH;
  red[g * WN_CH + c] = v;
  __syncthreads();
  for (int s = WN_RG / 2; s > 0; s >>= 1) {
    if (g < s) red[g * WN_CH + c] += red[(g + s) * WN_CH + c];
    __syncthreads();
  }
  const float t = red[c];
  __syncthreads();
  return t;
}

// Per-channel sums over the real rows (t < T, b < B) in two levels: block (channel tile, chunk g) sums its chunk of rows
// into part[g][c] (row strides, then the LDS tree), bn_finish_kernel adds the chunks in order.  MODE 0: y;  MODE 1: (y - mean)^2;
// MODE 2: dy into part, dy * xhat into part2.
template <int MODE>
__global__ __launch_bounds__(WN_CH* WN_RG) void bn_part_kernel(const float* __restrict__ y, const float* __restrict__ dy,
                                                               const float* __restrict__ mean, const float* __restrict__ var,
                                                               float eps, int N, int T, int B, int Bp, int chunk,
                                                               float* __restrict__ part, float* __restrict__ part2) {
  __shared__ float red[WN_RG * WN_CH];
  const int c = blockIdx.x * WN_CH + threadIdx.x % WN_CH, g = threadIdx.x / WN_CH;
  const bool okc = c < N;
  const int n = T * B;
  const int i0 = blockIdx.y * chunk, i1 = min(n, i0 + chunk);
  float s = 0.f, q = 0.f;
  if (okc) {
    const float mu = MODE ? mean[c] : 0.f;
    const float rs = MODE == 2 ? wn_rstd(var[c], eps) : 0.f;
    for (int i = i0 + g; i < i1; i += WN_RG) {
      const size_t j = ((size_t)(i / B) * Bp + i % B) * N + c;
      if (MODE == 0) {
        s += y[j];
      } else if (MODE == 1) {
        const float d = y[j] - mu;
        s += d * d;
      } else {
        const float d = dy[j];
        s += d;
        q += d * ((y[j] - mu) * rs);
      }
    }
  }
  const float ts = block_colsum(s, red);
  const float tq = MODE == 2 ? block_colsum(q, red) : 0.f;
  if (okc && g == 0) {
    part[(size_t)blockIdx.y * N + c] = ts;
    if (MODE == 2) part2[(size_t)blockIdx.y * N + c] = tq;
  }
}

// MODE 0: mean = sum / n;  MODE 1: var = sum / n, vup (Bessel-corrected when asked);  MODE 2: dbeta, dgamma
template <int MODE>
__global__ __launch_bounds__(256) void bn_finish_kernel(const float* __restrict__ part, const float* __restrict__ part2,
                                                        int G, int N, int n, int bessel, float* __restrict__ o1,
                                                        float* __restrict__ o2) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= N) return;
  float s = 0.f, q = 0.f;
  for (int g = 0; g < G; ++g) {
    s += part[(size_t)g * N + c];
    if (MODE == 2) q += part2[(size_t)g * N + c];
  }
  if (MODE == 0) {
    o1[c] = s / (float)n;
  } else if (MODE == 1) {
    const float v = s / (float)n;
    o1[c] = v;
    o2[c] = bessel ? v * ((float)n / (float)(n > 1 ? n - 1 : 1)) : v;
  } else {
    o1[c] = s;
    o2[c] = q;
  }
}

__global__ __launch_bounds__(256) void bn_tanh_kernel(const float* __restrict__ y, const float* __restrict__ mean,
                                                      const float* __restrict__ var, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float eps, float* __restrict__ out,
                                                      const float* __restrict__ zin, float* __restrict__ znext,
                                                      float* __restrict__ skip, int skip_first, int R, int B, int Bp, int D) {
  const int64_t n = (int64_t)R * D;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % D);
    const int b = (int)((i / D) % Bp);
    float o = 0.f;
    if (b < B) o = tanhf(gamma[c] * ((y[i] - mean[c]) * wn_rstd(var[c], eps)) + beta[c]);
    out[i] = o;
    if (znext) znext[i] = b < B ? o + zin[i] : 0.f;
    if (skip) skip[i] = skip_first ? o : skip[i] + o;
  }
}

__global__ __launch_bounds__(256) void bn_gate_kernel(const float* __restrict__ y, const float* __restrict__ mean,
                                                      const float* __restrict__ var, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float eps, float* __restrict__ fg,
                                                      float* __restrict__ p, int R, int B, int Bp, int D) {
  const int64_t n = (int64_t)R * D;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % D);
    const int64_t r = i / D;
    const int b = (int)(r % Bp);
    float f = 0.f, g = 0.f;
    if (b < B) {
      const size_t jf = (size_t)r * 2 * D + c, jg = jf + D;
      f = tanhf(gamma[c] * ((y[jf] - mean[c]) * wn_rstd(var[c], eps)) + beta[c]);
      g = wn_sigmoid(gamma[D + c] * ((y[jg] - mean[D + c]) * wn_rstd(var[D + c], eps)) + beta[D + c]);
    }
    fg[(size_t)r * 2 * D + c] = f;
    fg[(size_t)r * 2 * D + D + c] = g;
    p[i] = f * g;
  }
}

__global__ __launch_bounds__(256) void dtanh_kernel(float* __restrict__ dy, const float* __restrict__ d1,
                                                    const float* __restrict__ d2, const float* __restrict__ out, int R,
                                                    int B, int Bp, int D) {
  const int64_t n = (int64_t)R * D;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)((i / D) % Bp);
    const float o = out[i];
    const float u = d2 ? d1[i] + d2[i] : d1[i];
    dy[i] = b < B ? u * (1.f - o * o) : 0.f;
  }
}

__global__ __launch_bounds__(256) void dgate_kernel(float* __restrict__ dy, const float* __restrict__ dp,
                                                    const float* __restrict__ fg, int R, int B, int Bp, int D) {
  const int64_t n = (int64_t)R * D;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % D);
    const int64_t r = i / D;
    const int b = (int)(r % Bp);
    const size_t jf = (size_t)r * 2 * D + c, jg = jf + D;
    const float f = fg[jf], g = fg[jg], d = dp[i];
    dy[jf] = b < B ? d * g * (1.f - f * f) : 0.f;
    dy[jg] = b < B ? d * f * (g * (1.f - g)) : 0.f;
  }
}

__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(float* __restrict__ dy, const float* __restrict__ y,
                                                           const float* __restrict__ mean, const float* __restrict__ var,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ dbeta,
                                                           const float* __restrict__ dgamma, float eps, int N, int R,
                                                           int B, int Bp, float inv_n) {
  const int64_t n = (int64_t)R * N;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % N);
    const int b = (int)((i / N) % Bp);
    const float rs = wn_rstd(var[c], eps);
    const float xh = (y[i] - mean[c]) * rs;
    dy[i] = b < B ? gamma[c] * rs * (dy[i] - dbeta[c] * inv_n - xh * (dgamma[c] * inv_n)) : 0.f;
  }
}

__global__ __launch_bounds__(256) void bn_update_kernel(float* __restrict__ mm, float* __restrict__ mv,
                                                        float* __restrict__ biased, const float* __restrict__ mean,
                                                        const float* __restrict__ v, int n, float omd, float debias) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float bs = biased[i] - (biased[i] - mean[i]) * omd;
    biased[i] = bs;
    mm[i] = bs / debias;
    mv[i] = mv[i] - (mv[i] - v[i]) * omd;
  }
}

}  // namespace

void launch_wn_im2col(const float* z, float* col, const WnRows& rw, int D, int KS, int rate, hipStream_t st) {
  hipLaunchKernelGGL(im2col_kernel, dim3(grid_for((int64_t)rw.R() * KS * D / 4)), dim3(256), 0, st, z, col, rw.R(), rw.Bp,
                     D, KS, rate);
}

void launch_wn_col2im_add(const float* dcol, float* dz, const WnRows& rw, int D, int KS, int rate, hipStream_t st) {
  hipLaunchKernelGGL(col2im_add_kernel, dim3(grid_for((int64_t)rw.R() * D / 4)), dim3(256), 0, st, dcol, dz, rw.R(), rw.Bp,
                     D, KS, rate);
}

int wn_stat_chunks(const WnRows& rw) {
  const int n = rw.T * rw.B;
  return std::min(WN_MAX_CHUNKS, std::max(1, (n + 255) / 256));
}

namespace {
void bn_sums(int mode, const float* y, const float* dy, const float* mean, const float* var, float eps, int N, const WnRows& rw,
             float* ws, hipStream_t st) {
  const int n = rw.T * rw.B, G = wn_stat_chunks(rw), chunk = (n + G - 1) / G;
  const dim3 grid((N + WN_CH - 1) / WN_CH, G), block(WN_CH * WN_RG);
  float* part2 = ws + (size_t)G * N;
  if (mode == 0) hipLaunchKernelGGL(bn_part_kernel<0>, grid, block, 0, st, y, dy, mean, var, eps, N, rw.T, rw.B, rw.Bp, chunk, ws, part2);
  else if (mode == 1) hipLaunchKernelGGL(bn_part_kernel<1>, grid, block, 0, st, y, dy, mean, var, eps, N, rw.T, rw.B, rw.Bp, chunk, ws, part2);
  else hipLaunchKernelGGL(bn_part_kernel<2>, grid, block, 0, st, y, dy, mean, var, eps, N, rw.T, rw.B, rw.Bp, chunk, ws, part2);
}
}  // namespace

void launch_wn_bn_stats(const float* y, int N, const WnRows& rw, bool bessel, float* mean, float* var, float* vup, float* ws,
                        hipStream_t st) {
  const int n = rw.T * rw.B, G = wn_stat_chunks(rw);
  bn_sums(0, y, nullptr, nullptr, nullptr, 0.f, N, rw, ws, st);
  hipLaunchKernelGGL(bn_finish_kernel<0>, dim3((N + 255) / 256), dim3(256), 0, st, ws, nullptr, G, N, n, 0, mean, nullptr);
  bn_sums(1, y, nullptr, mean, nullptr, 0.f, N, rw, ws, st);
  hipLaunchKernelGGL(bn_finish_kernel<1>, dim3((N + 255) / 256), dim3(256), 0, st, ws, nullptr, G, N, n, bessel ? 1 : 0, var, vup);
}

void launch_wn_bn_tanh(const float* y, const float* mean, const float* var, const float* gamma, const float* beta, float eps,
                       float* out, const float* zin, float* znext, float* skip, bool skip_first, const WnRows& rw, int D,
                       hipStream_t st) {
  hipLaunchKernelGGL(bn_tanh_kernel, dim3(grid_for((int64_t)rw.R() * D)), dim3(256), 0, st, y, mean, var, gamma, beta, eps,
                     out, zin, znext, skip, skip_first ? 1 : 0, rw.R(), rw.B, rw.Bp, D);
}

void launch_wn_bn_gate(const float* y, const float* mean, const float* var, const float* gamma, const float* beta, float eps,
                       float* fg, float* p, const WnRows& rw, int D, hipStream_t st) {
  hipLaunchKernelGGL(bn_gate_kernel, dim3(grid_for((int64_t)rw.R() * D)), dim3(256), 0, st, y, mean, var, gamma, beta, eps,
                     fg, p, rw.R(), rw.B, rw.Bp, D);
}

void launch_wn_dtanh(float* dy, const float* d1, const float* d2, const float* out, const WnRows& rw, int D, hipStream_t st) {
  hipLaunchKernelGGL(dtanh_kernel, dim3(grid_for((int64_t)rw.R() * D)), dim3(256), 0, st, dy, d1, d2, out, rw.R(), rw.B,
                     rw.Bp, D);
}

void launch_wn_dgate(float* dy, const float* dp, const float* fg, const WnRows& rw, int D, hipStream_t st) {
  hipLaunchKernelGGL(dgate_kernel, dim3(grid_for((int64_t)rw.R() * D)), dim3(256), 0, st, dy, dp, fg, rw.R(), rw.B, rw.Bp, D);
}

void launch_wn_bn_bwd_sums(const float* y, const float* dy, const float* mean, const float* var, float eps, int N,
                           const WnRows& rw, float* dbeta, float* dgamma, float* ws, hipStream_t st) {
  const int G = wn_stat_chunks(rw);
  bn_sums(2, y, dy, mean, var, eps, N, rw, ws, st);
  hipLaunchKernelGGL(bn_finish_kernel<2>, dim3((N + 255) / 256), dim3(256), 0, st, ws, ws + (size_t)G * N, G, N, 0, 0, dbeta,
                     dgamma);
}

void launch_wn_bn_bwd_apply(float* dy, const float* y, const float* mean, const float* var, const float* gamma,
                            const float* dbeta, const float* dgamma, float eps, int N, const WnRows& rw, hipStream_t st) {
  hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(grid_for((int64_t)rw.R() * N)), dim3(256), 0, st, dy, y, mean, var, gamma,
                     dbeta, dgamma, eps, N, rw.R(), rw.B, rw.Bp, 1.f / (float)(rw.T * rw.B));
}

void launch_wn_bn_update(float* mm, float* mv, float* biased, const float* mean, const float* v, int n, float omd,
                         int64_t count, hipStream_t st) {
  // zero_debias_moving_mean: the divisor 1 - decay^count in fp32, as TF's pow on the float32 decay tensor
  const float debias = 1.f - powf(1.f - omd, (float)count);
  hipLaunchKernelGGL(bn_update_kernel, dim3(grid_for(n)), dim3(256), 0, st, mm, mv, biased, mean, v, n, omd, debias);
}

}  // namespace nasr
