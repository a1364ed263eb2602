// wave_aug.hip — the waveform augmentation kernels (the reference has no counterpart, the rules are at
// nasr_wave_aug in include/nasr.h).  Three launches cover a whole batch, between the resampler and mfcc_spectral_kernel:
//   wave_fir_kernel   one workgroup per tile of WV_TILE outputs of one utterance (the host's tile table): the direct-form
//                     FIR y[t] = sum_k h[k] x[t-k] in float32 on the vector ALUs.  A thread owns 8 consecutive outputs
//                     and keeps the 16 samples that 8 consecutive taps touch in registers; taps are taken WV_KC at a time:
//                     the chunk's taps and the x segment they reach (tile + WV_KC samples) are staged in LDS, the taps
//                     read from there as wave-uniform 16-byte loads, the samples 8 per 8 taps.  One accumulator per
//                     output, taps in ascending order, one FMA each: the order is a function of the output alone.
//                     An utterance without an RIR is copied.  Out of place.  A tile of an utterance with noise also
//                     leaves its share of Ps = sum y^2 and Pn = sum n^2, in float64: a thread's 8 samples in order, then a
//                     tree over the 128 threads - y is still in registers, so the powers cost no pass over memory
//   wave_gain_kernel  one workgroup per utterance with noise: the tiles' shares summed in float64 (thread i takes the
//                     tiles i, i + 256, ... in order, then a tree), g = sqrt(Ps/Pn) * scale rounded once to float32, 0
//                     when either power is 0.  The order of both sums depends on the utterance's length alone
//   wave_mix_kernel   the tiles again: z[t] = y[t] + g n[t], product rounded, then the sum; in place.  Tiles of an utterance
//                     without noise, or with g = 0, are left as they are.
// No atomics: every value has one writer, so an utterance's result does not depend on the rest of the batch.
#include "wave_aug.h"

namespace nasr_impl {

namespace {

constexpr int WV_KC = 512;                          // taps per chunk
constexpr int WV_SEG = WV_TILE + WV_KC;             // samples a chunk's taps reach from the tile, and one in front
constexpr int WV_SEG_LDS = WV_SEG / 8 * 12;         // with 4 pad words per 8 samples
constexpr int WV_GAIN_THREADS = 256;
static_assert(WV_PER_THREAD == 8 && WV_KC % 16 == 0, "the FIR's register window is 8 outputs x 8 taps, two groups per turn");

// 8 consecutive floats at a 16-byte aligned address
__device__ __forceinline__ void load8(float (&v)[8], const float* __restrict__ p) {
  const float4 lo = *reinterpret_cast<const float4*>(p), hi = *reinterpret_cast<const float4*>(p + 4);
  v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w;
  v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
}

// 8 taps h[0..8) at k .. k+7 on the 8 outputs of a thread: b holds x[T0-k .. T0-k+7], a the 8 samples in front of them
__device__ __forceinline__ void fir_group(float (&acc)[8], const float* __restrict__ h, const float (&a)[8], const float (&b)[8]) {
  const float4 h0 = *reinterpret_cast<const float4*>(h), h1 = *reinterpret_cast<const float4*>(h + 4);
  const float hv[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = fmaf(hv[i], j >= i ? b[j - i] : a[8 + j - i], acc[j]);
}

__global__ __launch_bounds__(WV_THREADS) void wave_fir_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                              const WvUtt* __restrict__ utt, const WvTile* __restrict__ tiles,
                                                              const float* __restrict__ taps, const float* __restrict__ clips,
                                                              double* __restrict__ part) {
  // sample i of the segment lives at word 12 (i / 8) + i % 8: the 8-sample groups of consecutive threads start 12 words
  // apart, 16-byte aligned, so a group is two ds_read_b128 and 16 consecutive lanes cover the 64 banks once
  __shared__ __align__(16) float sx[WV_SEG_LDS];
  __shared__ __align__(16) float sh[WV_KC];
  __shared__ double red[2][WV_THREADS];
  const WvTile tl = tiles[blockIdx.x];
  const WvUtt u = utt[tl.u];
  const int tid = threadIdx.x;
  const float* xs = x + u.off;
  float* ys = y + u.off;
  const int64_t tb = tl.t0;
  const int64_t T0 = tb + WV_PER_THREAD * tid;
  // taps k > t reach in front of the utterance: the tile's last output bounds the taps it needs
  const int64_t tend = tb + WV_TILE < u.n ? tb + WV_TILE : u.n;
  const int kend = (int)(tend < u.K ? tend : u.K);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (u.K == 0) {                                   // no RIR: the bits of the input
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (T0 + j < u.n) acc[j] = xs[T0 + j];
  }
  for (int k0 = 0; k0 < kend; k0 += WV_KC) {
    __syncthreads();                                // the chunk before has been read
    for (int i = tid; i < WV_KC; i += WV_THREADS) sh[i] = k0 + i < u.K ? taps[u.h_off + k0 + i] : 0.f;
    const int64_t base = tb - k0 - WV_KC;           // segment sample i is x[base + i]; zeros outside the utterance
    for (int i = tid; i < WV_SEG; i += WV_THREADS) {
      const int64_t g = base + i;
      sx[12 * (i >> 3) + (i & 7)] = (g >= 0 && g < u.n) ? xs[g] : 0.f;
    }
    __syncthreads();
    const int left = kend - k0 < WV_KC ? kend - k0 : WV_KC;
    const int ng = (left + 15) / 16 * 2;            // groups of 8 taps, two per turn; the taps past K are zeros
    // group 0 of the chunk: b = x[T0 - k0 .. + 7] = segment samples 8 (tid + WV_KC / 8) + j
    int p = 12 * (tid + WV_KC / 8);
    float a[8], b[8];
    load8(b, sx + p);
    for (int g = 0; g < ng; g += 2) {
      p -= 12;
      load8(a, sx + p);
      fir_group(acc, sh + 8 * g, a, b);
      p -= 12;
      load8(b, sx + p);
      fir_group(acc, sh + 8 * g + 8, b, a);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (T0 + j < u.n) ys[T0 + j] = acc[j];
  if (u.noise < 0) return;                          // (the same for the whole workgroup)
  // the tile's share of Ps and Pn; a product of two float32 is exact in float64
  const float* c = clips + u.c_off;
  int64_t idx = (u.c_pos + T0) % u.c_len;           // (o + t) mod L, carried from sample to sample
  double ps = 0.0, pn = 0.0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (T0 + j < u.n) {
      const double v = acc[j], w = c[idx];
      ps += v * v;
      pn += w * w;
    }
    if (++idx == u.c_len) idx = 0;
  }
  red[0][tid] = ps;
  red[1][tid] = pn;
  __syncthreads();
  for (int s = WV_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[0][tid] += red[0][tid + s];
      red[1][tid] += red[1][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    part[2 * (int64_t)blockIdx.x] = red[0][0];
    part[2 * (int64_t)blockIdx.x + 1] = red[1][0];
  }
}

__global__ __launch_bounds__(WV_GAIN_THREADS) void wave_gain_kernel(const double* __restrict__ part, const WvUtt* __restrict__ utt,
                                                                    float* __restrict__ gain) {
  __shared__ double rs[WV_GAIN_THREADS], rn[WV_GAIN_THREADS];
  const WvUtt u = utt[blockIdx.x];
  const int tid = threadIdx.x;
  if (u.noise < 0) {                                // (the same for the whole workgroup)
    if (tid == 0) gain[blockIdx.x] = 0.f;
    return;
  }
  const double* p = part + 2 * u.tile0;             // the utterance's tiles stand together in the table
  const int64_t nt = (u.n + WV_TILE - 1) / WV_TILE;
  double ps = 0.0, pn = 0.0;
  for (int64_t i = tid; i < nt; i += WV_GAIN_THREADS) {
    ps += p[2 * i];
    pn += p[2 * i + 1];
  }
  rs[tid] = ps;
  rn[tid] = pn;
  __syncthreads();
  for (int s = WV_GAIN_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      rs[tid] += rs[tid + s];
      rn[tid] += rn[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double Ps = rs[0], Pn = rn[0];
    gain[blockIdx.x] = (Ps == 0.0 || Pn == 0.0) ? 0.f : (float)(sqrt(Ps / Pn) * u.scale);
  }
}

__global__ __launch_bounds__(WV_THREADS) void wave_mix_kernel(float* __restrict__ y, const WvUtt* __restrict__ utt,
                                                              const WvTile* __restrict__ tiles, const float* __restrict__ clips,
                                                              const float* __restrict__ gain) {
  const WvTile tl = tiles[blockIdx.x];
  const WvUtt u = utt[tl.u];
  if (u.noise < 0) return;
  const float g = gain[tl.u];
  if (g == 0.f) return;                             // silence on either side: the bits stay
  const int tid = threadIdx.x;
  float* ys = y + u.off;
  const float* c = clips + u.c_off;
  int64_t idx = (u.c_pos + tl.t0 + tid) % u.c_len;
  const int64_t step = WV_THREADS % u.c_len;
  for (int i = tid; i < WV_TILE; i += WV_THREADS) {
    const int64_t t = tl.t0 + i;
    if (t < u.n) {
#pragma clang fp contract(off)
      const float gn = g * c[idx];                  // rounded before it is added: z = fl(y + fl(g n))
      ys[t] = ys[t] + gn;
    }
    idx += step;
    if (idx >= u.c_len) idx -= u.c_len;
  }
}

}  // namespace

void wave_tiles(WavePlan* p) {
  p->tiles.clear();
  for (size_t i = 0; i < p->utt.size(); ++i) {
    p->utt[i].tile0 = (int64_t)p->tiles.size();
    for (int64_t t0 = 0; t0 < p->utt[i].n; t0 += WV_TILE) p->tiles.push_back(WvTile{t0, (int32_t)i, 0});
  }
}

void launch_wave_aug(const float* x, float* y, const WvUtt* utt, int n, const WvTile* tiles, int64_t ntiles, const float* taps,
                     const float* clips, double* part, float* gain, hipStream_t st) {
  wave_fir_kernel<<<dim3((unsigned)ntiles), dim3(WV_THREADS), 0, st>>>(x, y, utt, tiles, taps, clips, part);
  wave_gain_kernel<<<dim3((unsigned)n), dim3(WV_GAIN_THREADS), 0, st>>>(part, utt, gain);
  wave_mix_kernel<<<dim3((unsigned)ntiles), dim3(WV_THREADS), 0, st>>>(y, utt, tiles, clips, gain);
}

}  // namespace nasr_impl
