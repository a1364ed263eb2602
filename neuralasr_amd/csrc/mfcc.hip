// mfcc.hip — the feature front end (reference utils.py:24-31, convert_to_mfcc): python_speech_features 0.6's
// mfcc(nfilt=128) on float32 audio, include_context and the whole-utterance normalisation, for a batch of utterances;
// or psf's logfbank in the place of mfcc (cfg.kind = 1), and psf's delta(feat, 2) columns appended (cfg.deltas).
//   mfcc_spectral_kernel  one wave per frame, every frame of the batch in one launch: pre-emphasis (float32, as the
//                         reference), then in float64 the 512-point real FFT (a 256-point complex FFT over the packed
//                         even / odd samples, radix-4 Stockham in LDS), power, energy, the sparse triangular filterbank,
//                         log, DCT-II with the lifter folded in, c0 <- log(energy); kind 1 writes the log filterbank
//                         energies themselves.  float64 so that narrow filters over near-zero bins keep their precision
//                         (at 8 kHz filter 0 is the DC bin alone).  Rows of the cep buffer are D =
//                         numcep (1 + deltas) wide, [static | delta | delta-delta]; this kernel writes the static part
//   mfcc_delta_kernel     one thread per (frame, static column) of the batch: one level of psf's delta(feat, 2) from
//                         one block of columns into the next, clamped to the frame's own utterance; launched once per
//                         level, so the delta-delta reads deltas that an earlier launch finished
//   mfcc_norm_kernel      one workgroup per utterance: the float64 mean and std of the stacked matrix from the centre
//                         frames (each counted once per window that holds it, the zero pads as a count), then the
//                         normalised rows written straight into the stacked layout
//   mfcc_norm_slot_kernel the same statistics, written as a model handle's batch slot takes them (nasr_batch.hip):
//                         the normalised centre frames [B][T][D] of a whole batch, zeros past each utterance's
//                         end, and one pad value (0 - mean) / std per utterance; nasr_upload_batch_audio
//   mfcc_causal_norm_kernel, mfcc_causal_slot_kernel
//                         cfg.norm = 1 (the reference has no causal front end): the same two output forms
//                         under the causal rule.  One workgroup per utterance: the per-frame sums p1, p2 in parallel over
//                         frames, their prefix sums S1, S2 by ONE lane each in frame order, then frame u normalised with
//                         the statistics of its first n_u = min(T, max(u+1, M)) frames; context frames outside the
//                         utterance are exact zeros
//   mfcc_stream_*_kernel  a stream session that takes samples (nasr_stream_feed_audio): per slot the carried sample tail and
//                         the new samples become one segment (assemble), mfcc_spectral_kernel runs on the newly complete
//                         frames, the prefix continues from the carried sums and the frames that have become normalisable
//                         are normalised (norm), the chunk's stacked rows go straight into the batch slot (stack), and the
//                         ring of the last 2 nc normalised frames and the tail are left for the next feed (carry)
// Tables (twiddles, filter weights, the DCT x lifter matrix) are built once per handle on the host in double.
// nasr_featurize_rates first resamples utterances at other rates to the config rate (resample.hip) into a device
// buffer, which the same two kernels then read.  A call with waveform augmentation runs wave_aug.hip's
// three kernels behind the resampler, and the spectral kernel reads their output.
#include "nasr_ctx.h"
#include "resample.h"

using namespace nasr;
using namespace nasr_impl;

namespace {

constexpr int FFT_N = 256;              // complex points: nfft = 512 real samples
constexpr int NBIN = 257;               // nfft/2 + 1
constexpr int MAX_FILT = 128;
constexpr int SPEC_WAVES = 4;           // frames per workgroup
constexpr int NORM_THREADS = 256;
constexpr double F64_EPS = 2.220446049250313e-16;   // numpy.finfo(float).eps: psf's stand-in for exact zeros

struct FzDims {
  int frame_len, frame_step, numcep, nfilt, nc;
  int append_energy;
  float preemph;
  int kind, width;                      // cfg.kind; D = numcep (1 + deltas), the row stride of the cep buffer
};

// ---------------------------------------------------------------------------------------------------------- kernels
// tw [256] = exp(-2 pi i t / 256), tw2 [257] = exp(-2 pi i k / 512); fb_lo/fb_n [nfilt]: a filter's first bin and bin
// count, fb_off [nfilt]: where its weights start in fb_w; dct [nfilt][numcep]: ortho DCT-II x lifter, c fastest.
// meta: uoff [n+1] (int64 sample offsets), foff [n+1] (int64 frame offsets), fmap [F] (int32 frame -> utterance).
// ulead (NULL: zeros) [n]: the samples of utterance u in front of its first frame of this launch: a stream session hands
// over the one sample that pre-emphasis reads before the frame (sample 0 of the BUFFER is the utterance's first only then).
__global__ __launch_bounds__(64 * SPEC_WAVES) void mfcc_spectral_kernel(
    const float* __restrict__ audio, const int64_t* __restrict__ uoff, const int64_t* __restrict__ foff,
    const int* __restrict__ fmap, const int64_t* __restrict__ ulead, int64_t nframes, const double2* __restrict__ tw,
    const double2* __restrict__ tw2, const int* __restrict__ fb_lo, const int* __restrict__ fb_n, const int* __restrict__ fb_off,
    const double* __restrict__ fb_w, const double* __restrict__ dct, FzDims d, double* __restrict__ cep) {
  __shared__ double2 buf[SPEC_WAVES][2][FFT_N];
  __shared__ double logmel[SPEC_WAVES][MAX_FILT];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t f = (int64_t)blockIdx.x * SPEC_WAVES + wv;
  const bool valid = f < nframes;        // wave-uniform; invalid waves still take every barrier
  double2* x = buf[wv][0];
  double2* y = buf[wv][1];

  // pre-emphasised samples of the frame, packed: x[m] = s[2m] + i s[2m+1]
  int64_t base = 0, len = 0, t0 = 0;
  if (valid) {
    const int u = fmap[f];
    base = uoff[u];
    len = uoff[u + 1] - base;
    t0 = (f - foff[u]) * (int64_t)d.frame_step + (ulead ? ulead[u] : 0);
  }
  const int nval = min(d.frame_len, 2 * FFT_N);   // frames longer than nfft are truncated (rfft(frame, nfft))
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = lane + 64 * r;
    float v[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int i = 2 * m + q;
      const int64_t g = t0 + i;
      float s = 0.f;
      if (valid && i < nval && g < len) {
        // s[g] = fl(x[g] - fl(preemph * x[g-1])): two roundings (psf preemphasis on float32).  HIP's __fmul_rn and
        // __fsub_rn are plain operators, which the default -ffp-contract=fast-honor-pragmas fuses into one FMA
#pragma clang fp contract(off)
        const float cur = audio[base + g];
        s = g == 0 ? cur : cur - d.preemph * audio[base + g - 1];
      }
      v[q] = s;
    }
    x[m] = make_double2(v[0], v[1]);
  }
  __syncthreads();

  // 256-point complex FFT: four radix-4 Stockham stages, 64 butterflies each (one per lane), ping-pong x <-> y
#pragma unroll
  for (int p = 1, stride = FFT_N / 4; p < FFT_N; p *= 4, stride /= 4) {
    const int i = lane, k = i & (p - 1);
    const double2 a0 = x[i];
    double2 a1 = x[i + 64], a2 = x[i + 128], a3 = x[i + 192];
    const double2 w1 = tw[k * stride], w2 = tw[2 * k * stride], w3 = tw[3 * k * stride];
    a1 = make_double2(a1.x * w1.x - a1.y * w1.y, a1.x * w1.y + a1.y * w1.x);
    a2 = make_double2(a2.x * w2.x - a2.y * w2.y, a2.x * w2.y + a2.y * w2.x);
    a3 = make_double2(a3.x * w3.x - a3.y * w3.y, a3.x * w3.y + a3.y * w3.x);
    const double2 b0 = make_double2(a0.x + a2.x, a0.y + a2.y), b1 = make_double2(a0.x - a2.x, a0.y - a2.y);
    const double2 b2 = make_double2(a1.x + a3.x, a1.y + a3.y);
    const double2 b3 = make_double2(a1.y - a3.y, a3.x - a1.x);       // -i (a1 - a3)
    const int j = 4 * (i - k) + k;
    y[j] = make_double2(b0.x + b2.x, b0.y + b2.y);
    y[j + p] = make_double2(b1.x + b3.x, b1.y + b3.y);
    y[j + 2 * p] = make_double2(b0.x - b2.x, b0.y - b2.y);
    y[j + 3 * p] = make_double2(b1.x - b3.x, b1.y - b3.y);
    __syncthreads();
    double2* tmp = x; x = y; y = tmp;
  }

  // the real spectrum X[k] = E[k] + W512^k O[k], E = (Z[k] + conj Z[N-k]) / 2, O = (Z[k] - conj Z[N-k]) / 2i; power
  // |X[k]|^2 / 512 into y (as doubles), and the frame energy (their sum, fixed order)
  double* pw = reinterpret_cast<double*>(y);
  double en = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int k = lane + 64 * r;
    const double2 zk = x[k], zn = x[(FFT_N - k) & (FFT_N - 1)];
    double re, im;
    if (k == 0) {
      re = zk.x + zk.y;
      im = 0.0;
    } else {
      const double er = 0.5 * (zk.x + zn.x), ei = 0.5 * (zk.y - zn.y);
      const double orr = 0.5 * (zk.y + zn.y), oi = -0.5 * (zk.x - zn.x);
      const double2 w = tw2[k];
      re = er + (orr * w.x - oi * w.y);
      im = ei + (orr * w.y + oi * w.x);
    }
    const double p = (re * re + im * im) * (1.0 / 512.0);
    pw[k] = p;
    en += p;
  }
  if (lane == 0) {                        // X[256] = Re Z[0] - Im Z[0]
    const double re = x[0].x - x[0].y;
    const double p = re * re * (1.0 / 512.0);
    pw[FFT_N] = p;
    en += p;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) en += __shfl_xor(en, o);
  __syncthreads();

  // filterbank: filter j = lane, lane + 64 sums its own bins; exact zeros (empty filters, digital silence) -> eps
  for (int j = lane; j < d.nfilt; j += 64) {
    const int lo = fb_lo[j], n = fb_n[j];
    const double* w = fb_w + fb_off[j];
    double acc = 0.0;
    for (int i = 0; i < n; ++i) acc += w[i] * pw[lo + i];
    logmel[wv][j] = log(acc == 0.0 ? F64_EPS : acc);
  }
  __syncthreads();

  // DCT-II (ortho) x lifter; c0 <- log(energy).  kind 1 (numcep == nfilt): the log filterbank energies as they are
  if (valid) {
    double* row = cep + f * d.width;
    if (d.kind == 1) {
      for (int j = lane; j < d.numcep; j += 64) row[j] = logmel[wv][j];
    } else {
      const double lg_en = log(en == 0.0 ? F64_EPS : en);
      for (int c = lane; c < d.numcep; c += 64) {
        double acc = 0.0;
        for (int j = 0; j < d.nfilt; ++j) acc += dct[j * d.numcep + c] * logmel[wv][j];
        row[c] = (c == 0 && d.append_energy) ? lg_en : acc;
      }
    }
  }
}

// One level of psf 0.6's delta(feat, N=2) over the packed frames [F][width] of the batch: columns [src, src + numcep)
// of every frame give columns [dst, dst + numcep).  p is the source edge-replicated inside the frame's own utterance
// (t clamped to [foff[u], foff[u+1])), and the sum is taken in this order:
//   delta[t] = ((p[t+1] - p[t-1]) + 2 (p[t+2] - p[t-2])) / 10
// Consecutive threads take consecutive columns of a frame.  A launch reads only columns that an earlier launch wrote:
// the delta-delta is a second launch with src = the delta columns, so its edges replicate the DELTA array.
__global__ __launch_bounds__(NORM_THREADS) void mfcc_delta_kernel(double* cep, const int64_t* __restrict__ foff,
                                                                  const int* __restrict__ fmap, int64_t nframes, int numcep,
                                                                  int width, int src, int dst) {
  const int64_t e = (int64_t)blockIdx.x * NORM_THREADS + threadIdx.x;
  if (e >= nframes * numcep) return;
  const int64_t f = e / numcep;
  const int c = (int)(e - f * numcep);
  const int u = fmap[f];
  const int64_t lo = foff[u], hi = foff[u + 1] - 1;
  auto p = [&](int64_t t) { return cep[(t < lo ? lo : t > hi ? hi : t) * width + src + c]; };
  const double d1 = p(f + 1) - p(f - 1), d2 = p(f + 2) - p(f - 2);
  cep[f * width + dst + c] = (d1 + 2.0 * d2) / 10.0;
}

// One workgroup per utterance of T frames: the stacked matrix [T][W*C] (W = 2 nc + 1) holds centre frame t in
// cnt_t = min(t,nc) + min(T-1-t,nc) + 1 windows, zeros elsewhere.  Two float64 passes (numpy's mean, then the mean
// squared deviation), fixed-order sums.  Every thread of the workgroup calls it and gets the same (mean, std).
// `numcep`, here and in the two kernels below, is the width of a frame of the cep buffer: D = numcep (1 + deltas).
__device__ __forceinline__ void utt_mean_std(const double* __restrict__ src, int64_t T, int numcep, int nc, double* red,
                                             double* mean_out, double* sd_out) {
  const int tid = threadIdx.x;
  const int W = 2 * nc + 1;
  const int64_t ne = T * numcep;
  auto cnt = [&](int64_t t) { return (double)((t < nc ? t : nc) + (T - 1 - t < nc ? T - 1 - t : nc) + 1); };
  auto block_sum = [&](double v) {
    red[tid] = v;
    __syncthreads();
    for (int s = NORM_THREADS / 2; s > 0; s >>= 1) {
      if (tid < s) red[tid] += red[tid + s];
      __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
  };
  const double N = (double)T * W * numcep;
  double s = 0.0, slots = 0.0;
  for (int64_t e = tid; e < ne; e += NORM_THREADS) {
    const double c = cnt(e / numcep);
    s += c * src[e];
    slots += c;
  }
  const double mean = block_sum(s) / N;
  const double zeros = N - block_sum(slots);          // pad slots, each (0 - mean)^2
  double q = 0.0;
  for (int64_t e = tid; e < ne; e += NORM_THREADS) {
    const double dv = src[e] - mean;
    q += cnt(e / numcep) * dv * dv;
  }
  const double var = (block_sum(q) + zeros * mean * mean) / N;
  *mean_out = mean;
  *sd_out = sqrt(var);
}

// the one expression both writers round through: a stacked element, a centre frame's, a pad value (v = 0)
__device__ __forceinline__ float norm_value(double v, double mean, double sd) { return (float)((v - mean) / sd); }

// The stacked form: out[t][w*C + c] = (cep[t+w-nc][c] - mean) / std (0 outside the utterance), utterance after utterance.
__global__ __launch_bounds__(NORM_THREADS) void mfcc_norm_kernel(const double* __restrict__ cep,
                                                                 const int64_t* __restrict__ foff, int numcep, int nc,
                                                                 float* __restrict__ out, double* __restrict__ mstd) {
  __shared__ double red[NORM_THREADS];
  const int u = blockIdx.x, tid = threadIdx.x;
  const int64_t f0 = foff[u], T = foff[u + 1] - f0;
  const double* src = cep + f0 * numcep;
  double mean, sd;
  utt_mean_std(src, T, numcep, nc, red, &mean, &sd);
  if (mstd && tid == 0) {
    mstd[2 * u] = mean;
    mstd[2 * u + 1] = sd;
  }
  const int rowlen = (2 * nc + 1) * numcep;
  float* dst = out + f0 * rowlen;
  for (int64_t e = tid; e < T * rowlen; e += NORM_THREADS) {
    const int64_t t = e / rowlen;
    const int r = (int)(e - t * rowlen);
    const int64_t ts = t + r / numcep - nc;
    const double v = (ts >= 0 && ts < T) ? src[ts * numcep + r % numcep] : 0.0;
    dst[e] = norm_value(v, mean, sd);
  }
}

// The batch-slot form (the `centre` layout of nasr_upload_batch_context): centre [B][Tb][numcep] gets utterance u's
// normalised frames and exact zeros for t >= its T frames, pad[u] the value of an out-of-utterance context frame.
// Consecutive threads write consecutive floats of the utterance's [Tb][numcep] block.
__global__ __launch_bounds__(NORM_THREADS) void mfcc_norm_slot_kernel(const double* __restrict__ cep,
                                                                      const int64_t* __restrict__ foff, int numcep, int nc,
                                                                      int Tb, float* __restrict__ centre,
                                                                      float* __restrict__ pad) {
  __shared__ double red[NORM_THREADS];
  const int u = blockIdx.x, tid = threadIdx.x;
  const int64_t f0 = foff[u], T = foff[u + 1] - f0;
  const double* src = cep + f0 * numcep;
  double mean, sd;
  utt_mean_std(src, T, numcep, nc, red, &mean, &sd);
  if (tid == 0) pad[u] = norm_value(0.0, mean, sd);
  const int64_t ne = T * numcep, nb = (int64_t)Tb * numcep;
  float* dst = centre + (int64_t)u * nb;
  for (int64_t e = tid; e < nb; e += NORM_THREADS) dst[e] = e < ne ? norm_value(src[e], mean, sd) : 0.f;
}

// ------------------------------------------------------------------------------------------ the causal rule (§16)
// (mean, sd) of the first n frames from their sums S1 = sum x, S2 = sum x^2: the one expression every user of the rule
// rounds through.  No FMA: mean * mean is rounded before it is subtracted.  A variance that is not > 0 (digital silence,
// or a NaN) gives sd = 1, so that 0 / 0 becomes 0.
__device__ __forceinline__ void causal_mean_sd(double S1, double S2, int64_t n, int D, double* mean, double* sd) {
#pragma clang fp contract(off)
  const double N = (double)(n * D);
  const double m = S1 / N;
  const double var = S2 / N - m * m;
  *mean = m;
  *sd = var > 0.0 ? sqrt(var) : 1.0;
}

// the frames whose statistics normalise frame u of T: every frame waits for the first M, none looks past its own
__device__ __forceinline__ int64_t causal_count(int64_t u, int64_t T, int M) {
  const int64_t n = u + 1 > M ? u + 1 : M;
  return n < T ? n : T;
}

// One workgroup walks T frames [T][D] at src; every thread calls it.  pfx [T][2] receives (S1, S2) after each frame.
// Frames are taken NORM_THREADS at a time: each thread sums the columns of its frame in ascending order (product rounded,
// then added), lane 0 of wave 0 then walks the chunk's p1 and lane 0 of wave 1 its p2 in frame order, each carrying its
// running sum from chunk to chunk: the association order is that of a sequential loop over the utterance, whatever T is
// and wherever a stream session cuts it.  carry: the sum so far (thread 0: S1, thread 64: S2; 0 at the utterance's
// start); returned to those two threads as it stands after the T frames.  Every value has one writer.
__device__ __forceinline__ double causal_prefix(const double* __restrict__ src, int64_t T, int D, double carry, double* pfx,
                                                double (*sh)[NORM_THREADS]) {
  const int tid = threadIdx.x;
  for (int64_t base = 0; base < T; base += NORM_THREADS) {
    const int64_t u = base + tid;
    if (u < T) {
#pragma clang fp contract(off)
      const double* row = src + u * D;
      double a = 0.0, b = 0.0;
      for (int k = 0; k < D; ++k) {
        const double v = row[k];
        a += v;
        b += v * v;
      }
      sh[0][tid] = a;
      sh[1][tid] = b;
    }
    __syncthreads();
    if (tid == 0 || tid == 64) {
      double* q = sh[tid >> 6];
      const int cnt = (int)(T - base < NORM_THREADS ? T - base : NORM_THREADS);
      for (int i = 0; i < cnt; ++i) {
        carry += q[i];
        q[i] = carry;
      }
    }
    __syncthreads();
    if (u < T) {
      pfx[2 * u] = sh[0][tid];
      pfx[2 * u + 1] = sh[1][tid];
    }
  }
  __syncthreads();
  return carry;
}

// One workgroup per utterance of T frames: pfx [T][2] as above, ms [T][2] the (mean, sd) frame u is normalised with.
__device__ __forceinline__ void causal_utt_stats(const double* __restrict__ src, int64_t T, int D, int M, double* pfx,
                                                 double* ms, double (*sh)[NORM_THREADS]) {
  causal_prefix(src, T, D, 0.0, pfx, sh);
  for (int64_t u = threadIdx.x; u < T; u += NORM_THREADS) {
    const int64_t n = causal_count(u, T, M);
    double mean, sd;
    causal_mean_sd(pfx[2 * (n - 1)], pfx[2 * (n - 1) + 1], n, D, &mean, &sd);
    ms[2 * u] = mean;
    ms[2 * u + 1] = sd;
  }
  __syncthreads();
}

// The stacked form under the causal rule: out[t][w*D + c] = y[t+w-nc][c], exact 0 outside the utterance; mstd (nullable)
// gets (mean, sd) of all T frames.  pfx and ms are [F][2] scratch, indexed like the frames.
__global__ __launch_bounds__(NORM_THREADS) void mfcc_causal_norm_kernel(const double* __restrict__ cep,
                                                                        const int64_t* __restrict__ foff, int D, int nc, int M,
                                                                        double* pfx, double* ms, float* __restrict__ out,
                                                                        double* __restrict__ mstd) {
  __shared__ double sh[2][NORM_THREADS];
  const int u = blockIdx.x, tid = threadIdx.x;
  const int64_t f0 = foff[u], T = foff[u + 1] - f0;
  const double* src = cep + f0 * D;
  const double* m = ms + 2 * f0;
  causal_utt_stats(src, T, D, M, pfx + 2 * f0, ms + 2 * f0, sh);
  if (mstd && tid == 0) {                 // frame T-1 is normalised with all T frames
    mstd[2 * u] = m[2 * (T - 1)];
    mstd[2 * u + 1] = m[2 * (T - 1) + 1];
  }
  const int rowlen = (2 * nc + 1) * D;
  float* dst = out + f0 * rowlen;
  for (int64_t e = tid; e < T * rowlen; e += NORM_THREADS) {
    const int64_t t = e / rowlen;
    const int r = (int)(e - t * rowlen);
    const int64_t ts = t + r / D - nc;
    dst[e] = (ts >= 0 && ts < T) ? norm_value(src[ts * D + r % D], m[2 * ts], m[2 * ts + 1]) : 0.f;
  }
}

// The batch-slot form under the causal rule: the normalised centre frames, zeros past the utterance's end, pad value 0.
__global__ __launch_bounds__(NORM_THREADS) void mfcc_causal_slot_kernel(const double* __restrict__ cep,
                                                                        const int64_t* __restrict__ foff, int D, int M, int Tb,
                                                                        double* pfx, double* ms, float* __restrict__ centre,
                                                                        float* __restrict__ pad) {
  __shared__ double sh[2][NORM_THREADS];
  const int u = blockIdx.x, tid = threadIdx.x;
  const int64_t f0 = foff[u], T = foff[u + 1] - f0;
  const double* src = cep + f0 * D;
  const double* m = ms + 2 * f0;
  causal_utt_stats(src, T, D, M, pfx + 2 * f0, ms + 2 * f0, sh);
  if (tid == 0) pad[u] = 0.f;
  const int64_t ne = T * D, nb = (int64_t)Tb * D;
  float* dst = centre + (int64_t)u * nb;
  for (int64_t e = tid; e < nb; e += NORM_THREADS) {
    const int64_t t = e / D;
    dst[e] = e < ne ? norm_value(src[e], m[2 * t], m[2 * t + 1]) : 0.f;
  }
}

// ---------------------------------------------------------------------- a stream session that takes samples (§16)
// One feed, slot by slot (FzFeedSlot, worked out on the host): the slot's segment of the work buffer is its carried tail
// followed by its new samples.  grid (x, S).
__global__ __launch_bounds__(NORM_THREADS) void mfcc_stream_assemble_kernel(const FzFeedSlot* __restrict__ desc,
                                                                            const float* __restrict__ tail, int tail_cap,
                                                                            const float* __restrict__ in, float* __restrict__ seg) {
  const int b = blockIdx.y;
  const FzFeedSlot d = desc[b];
  const int64_t n = d.ntail + d.nnew;
  for (int64_t i = (int64_t)blockIdx.x * NORM_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * NORM_THREADS)
    seg[d.seg_off + i] = i < d.ntail ? tail[(int64_t)b * tail_cap + i] : in[d.in_off + i - d.ntail];
}

// One workgroup per slot, behind the spectral kernel: the sequential update of the slot's running sums over its new frames
// (causal_prefix, continued from sums [S][2]), then every frame that this feed makes normalisable - frames [nnorm, upto),
// the waiting ones of earlier feeds from pend [S][M][D] and the new ones from cep - through causal_mean_sd and norm_value
// with exactly S[n_u], n_u = max(u+1, M) capped by T when the feed completes the utterance; frames that still wait for
// the M-th go to pend.  ynew [.][D] receives the normalised frames in frame order.
__global__ __launch_bounds__(NORM_THREADS) void mfcc_stream_norm_kernel(const double* __restrict__ cep,
                                                                        const FzFeedSlot* __restrict__ desc, int D, int M,
                                                                        double* sums, double* pend, double* pfx,
                                                                        float* __restrict__ ynew) {
  __shared__ double sh[2][NORM_THREADS];
  __shared__ double s0[2];
  const int b = blockIdx.x, tid = threadIdx.x;
  const FzFeedSlot d = desc[b];
  const int64_t nnew = d.want - d.nfb;
  const double* src = cep + d.f_off * D;
  double* px = pfx + 2 * d.f_off;
  double* pd = pend + (int64_t)b * M * D;
  const bool chain = tid == 0 || tid == 64;
  double c = 0.0;
  if (chain) {
    if (d.nfb > 0) c = sums[2 * b + (tid >> 6)];
    s0[tid >> 6] = c;                     // S[nfb]
  }
  c = causal_prefix(src, nnew, D, c, px, sh);
  if (chain) sums[2 * b + (tid >> 6)] = c;
  const int64_t ne = (d.upto - d.nnorm) * D;
  float* y = ynew + d.y_off * D;
  for (int64_t e = tid; e < ne; e += NORM_THREADS) {
    const int64_t j = e / D, u = d.nnorm + j;
    const int k = (int)(e - j * D);
    int64_t n = u + 1 > M ? u + 1 : M;
    if (d.T >= 0 && n > d.T) n = d.T;
    const double S1 = n > d.nfb ? px[2 * (n - d.nfb - 1)] : s0[0];
    const double S2 = n > d.nfb ? px[2 * (n - d.nfb - 1) + 1] : s0[1];
    double mean, sd;
    causal_mean_sd(S1, S2, n, D, &mean, &sd);
    const double x = u >= d.nfb ? src[(u - d.nfb) * D + k] : pd[u * D + k];
    y[e] = norm_value(x, mean, sd);
  }
  if (d.upto == 0)                        // fewer than M frames so far (want < M): they wait, at their own index
    for (int64_t e = tid; e < nnew * D; e += NORM_THREADS) pd[d.nfb * D + e] = src[e];
}

// The chunk's stacked rows [S][Tc][(2 nc + 1) D] straight into the batch slot, one thread per element: row t of slot b is
// row rows0 + t of its utterance, context frame s from this feed's ynew or, older, from the slot's ring yring [S][R][D]
// (frame s at s mod R); exact zeros outside the utterance and behind the slot's nrows.
__global__ __launch_bounds__(NORM_THREADS) void mfcc_stream_stack_kernel(const FzFeedSlot* __restrict__ desc, int S, int Tc, int D,
                                                                         int nc, int R, const float* __restrict__ ynew,
                                                                         const float* __restrict__ yring, float* __restrict__ out) {
  const int F = (2 * nc + 1) * D;
  const int64_t e = (int64_t)blockIdx.x * NORM_THREADS + threadIdx.x;
  if (e >= (int64_t)S * Tc * F) return;
  const int b = (int)(e / ((int64_t)Tc * F));
  const int64_t r = e - (int64_t)b * Tc * F;
  const int t = (int)(r / F), q = (int)(r - (int64_t)t * F);
  const int w = q / D, k = q - w * D;
  const FzFeedSlot d = desc[b];
  float v = 0.f;
  if (t < d.nrows) {
    const int64_t fs = d.rows0 + t + w - nc;
    if (fs >= 0 && fs < d.upto)
      v = fs >= d.nnorm ? ynew[(d.y_off + fs - d.nnorm) * D + k] : yring[((int64_t)b * R + fs % R) * D + k];
  }
  out[e] = v;
}

// One workgroup per slot, behind the stacking kernel (which reads the ring as the feed found it): the last 2 nc normalised
// frames into the ring, the un-framed samples (with the one in front of them) into the tail.
__global__ __launch_bounds__(NORM_THREADS) void mfcc_stream_carry_kernel(const FzFeedSlot* __restrict__ desc, int D, int nc, int R,
                                                                         const float* __restrict__ ynew, float* __restrict__ yring,
                                                                         const float* __restrict__ seg, float* __restrict__ tail,
                                                                         int tail_cap) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const FzFeedSlot d = desc[b];
  int64_t u0 = d.upto - 2 * nc;
  if (u0 < d.nnorm) u0 = d.nnorm;
  for (int64_t e = tid; e < (d.upto - u0) * D; e += NORM_THREADS) {
    const int64_t u = u0 + e / D;
    const int k = (int)(e % D);
    yring[((int64_t)b * R + u % R) * D + k] = ynew[(d.y_off + u - d.nnorm) * D + k];
  }
  for (int64_t i = tid; i < d.nkeep; i += NORM_THREADS) tail[(int64_t)b * tail_cap + i] = seg[d.seg_off + d.keep_off + i];
}

// --------------------------------------------------------------------------------------------------- host tables
bool cfg_ok(const nasr_mfcc_cfg* c, std::string* why) {
  if (!c) return *why = "null cfg", false;
  if (c->samplerate < 1) return *why = "samplerate must be >= 1", false;
  if (c->nfft != 2 * FFT_N) return *why = "only nfft = 512 (python_speech_features 0.6's default) is implemented", false;
  if (c->nfilt < 1 || c->nfilt > MAX_FILT) return *why = "nfilt must be in [1,128]", false;
  if (c->numcep < 1 || c->numcep > c->nfilt) return *why = "numcep must be in [1,nfilt]", false;
  if (c->kind != 0 && c->kind != 1) return *why = "kind must be 0 (MFCC) or 1 (log-mel filterbank)", false;
  if (c->deltas < 0 || c->deltas > 2) return *why = "deltas must be 0, 1 or 2", false;
  if (c->kind == 1 && c->numcep != c->nfilt)
    return *why = "kind 1 (log-mel filterbank): numcep is the number of filters and must equal nfilt", false;
  if (c->numcontext < 0) return *why = "numcontext must be >= 0", false;
  if (!(c->winlen > 0.0) || !(c->winstep > 0.0)) return *why = "winlen and winstep must be > 0", false;
  if (c->kind == 0 && c->ceplifter < 0) return *why = "ceplifter must be >= 0", false;
  if (c->norm != 0 && c->norm != 1) return *why = "norm must be 0 (whole utterance) or 1 (causal)", false;
  if (c->norm == 1 && (c->norm_min_frames < 1 || c->norm_min_frames > 1000))
    return *why = "norm_min_frames must be in [1,1000] when norm = 1", false;
  if (c->norm == 1 && c->deltas > 0)
    return *why = "norm = 1 (causal) needs deltas = 0: psf's delta looks 2 frames ahead (4 for the delta-delta) and replicates "
                  "the end of the array, which needs a look-ahead rule of its own",
           false;
  return true;
}

// psf round_half_up: Decimal(x).quantize(1, ROUND_HALF_UP) for x >= 0 (x - floor(x) is exact here)
int64_t round_half_up(double x) {
  const double fl = std::floor(x);
  return (int64_t)fl + (x - fl >= 0.5 ? 1 : 0);
}

int64_t frames_of(int64_t flen, int64_t fstep, int64_t n) {
  if (n <= flen) return 1;
  return 1 + (n - flen + fstep - 1) / fstep;   // 1 + ceil((n - frame_len) / frame_step)
}

// psf get_filterbanks(nfilt, nfft, samplerate, 0, samplerate/2): mel points by numpy.linspace, bins by floor
std::vector<double> filter_bins(const nasr_mfcc_cfg* c) {
  const int nf = c->nfilt;
  auto hz2mel = [](double hz) { return 2595.0 * std::log10(1.0 + hz / 700.0); };
  auto mel2hz = [](double mel) { return 700.0 * (std::pow(10.0, mel / 2595.0) - 1.0); };
  const double lo = hz2mel(0.0), hi = hz2mel(c->samplerate / 2.0);
  const double step = (hi - lo) / (nf + 1);
  std::vector<double> bin(nf + 2);
  for (int i = 0; i < nf + 2; ++i) {
    const double m = i == nf + 1 ? hi : i * step + lo;
    bin[i] = std::floor((c->nfft + 1) * mel2hz(m) / c->samplerate);
  }
  return bin;
}

// dense [nfilt][nfft/2+1] weights in double, as psf fills them
std::vector<double> filter_weights(const nasr_mfcc_cfg* c, const std::vector<double>& bin) {
  const int nb = c->nfft / 2 + 1;
  std::vector<double> w((size_t)c->nfilt * nb, 0.0);
  for (int j = 0; j < c->nfilt; ++j) {
    for (int i = (int)bin[j]; i < (int)bin[j + 1]; ++i) w[(size_t)j * nb + i] = (i - bin[j]) / (bin[j + 1] - bin[j]);
    for (int i = (int)bin[j + 1]; i < (int)bin[j + 2]; ++i) w[(size_t)j * nb + i] = (bin[j + 2] - i) / (bin[j + 2] - bin[j + 1]);
  }
  return w;
}

}  // namespace

namespace nasr_impl {

struct FzState {
  nasr_mfcc_cfg cfg;
  FzDims d;
  int W = 1;
  DevPtr<double2> tw, tw2;
  DevPtr<int> fb_lo, fb_n, fb_off;
  DevPtr<double> fb_w, dct;
  DevBuf audio, meta, cep, out, mstd;
  DevBuf pfx, fms;                     // norm = 1: the prefix sums (S1, S2) and the (mean, sd) of every frame, [F][2] each
  DevBuf sin, ynew;                    // a stream session's feed: the new samples as they came, the frames it normalises
  std::vector<char> hmeta;
  DevPtr<double2> rs_tab;              // the resampling filter's (table[k], table[k+1]) pairs, made at the first use
  DevBuf raud, rmeta;                  // resampled audio; the resampling plan (RsUtt [n], then RsWave [waves])
  std::vector<char> hrmeta;
  // waveform augmentation: the banks (set once, offsets [n+1] from 0 on the host), and a call's augmented
  // samples, its plan (WvUtt [n], then WvTile [tiles]), the tiles' powers [tiles][2] and the gains [n]; none of them exists
  // until a call asks for it
  DevBuf noise_bank, rir_bank;
  std::vector<int64_t> noise_off, rir_off;
  DevBuf wav, wmeta, wpart, gain;
  std::vector<char> hwmeta;
  Event ev[4];
  float times[3] = {0.f, 0.f, 0.f};
  bool times_pending = false;          // ev[0..2] were recorded by a batch-slot call and not read yet (nasr_featurize_times)
  // A batch-slot call (nasr_upload_batch_audio, nasr_stage_batch_audio) runs the front end on a MODEL handle's stream and
  // returns with the kernels still in flight: ev_busy marks the point behind which the scratch buffers above are free.
  Event ev_busy;
  bool busy_valid = false;
};

}  // namespace nasr_impl

void nasr_impl::FzStateDelete::operator()(FzState* f) const { delete f; }

namespace {

// Grows scratch buffer b to `bytes`.  A batch-slot call may still read the old allocation on a model's stream (ev_busy):
// the host waits for that event before the buffer is freed, so the free never races the kernels and does not lean on
// hipFree's own device-wide synchronisation.  Only a call LARGER than every one before it pays this wait; buffers that
// are big enough are ordered by scratch_acquire's stream wait alone.
bool scratch_ensure(FzState& z, DevBuf& b, size_t bytes) {
  if (bytes > b.cap && z.busy_valid) {
    (void)hipEventSynchronize(z.ev_busy);
    z.busy_valid = false;
  }
  return b.ensure(bytes, nullptr);
}

const RsWave* rs_waves(FzState& z, int n) {
  return reinterpret_cast<const RsWave*>(z.rmeta.as<char>() + (size_t)n * sizeof(RsUtt));
}

// the filter table (once per handle), the plan's host image and the device buffers of a resampling launch
int resample_prepare(nasr_ctx* h, FzState& z, const ResamplePlan& plan, int64_t in_samples) {
  if (!z.rs_tab) {
    const std::vector<double2> pairs = resample_table_pairs();
    HIPCHK(h, hipMalloc(z.rs_tab.out(), pairs.size() * sizeof(double2)));
    HIPCHK(h, hipMemcpy(z.rs_tab.get(), pairs.data(), pairs.size() * sizeof(double2), hipMemcpyHostToDevice));
  }
  const size_t ub = plan.utt.size() * sizeof(RsUtt), wb = plan.waves.size() * sizeof(RsWave);
  z.hrmeta.resize(ub + wb);
  memcpy(z.hrmeta.data(), plan.utt.data(), ub);
  memcpy(z.hrmeta.data() + ub, plan.waves.data(), wb);
  if (!scratch_ensure(z, z.audio, (size_t)in_samples * 4) || !scratch_ensure(z, z.raud, (size_t)plan.total * 4) ||
      !scratch_ensure(z, z.rmeta, z.hrmeta.size()))
    return h->fail(NASR_ERR_HIP, "resampling: device buffers for " + std::to_string(in_samples) + " + " +
                                     std::to_string(plan.total) + " samples could not be allocated");
  return NASR_OK;
}

// wait for the stream; the device-timed phases between the four events
int finish(nasr_ctx* h, FzState& z) {
  if (int rc = sync_checked(h)) return rc;
  for (int i = 0; i < 3; ++i)
    if (hipEventElapsedTime(&z.times[i], z.ev[i], z.ev[i + 1]) != hipSuccess) z.times[i] = 0.f;
  z.times_pending = false;
  return NASR_OK;
}

// `st` is about to use the scratch buffers: behind whatever batch-slot call still reads them on another stream
int scratch_acquire(nasr_ctx* eh, FzState& z, hipStream_t st) {
  if (!z.busy_valid) return NASR_OK;
  // The event was recorded on a model handle's stream, and that handle may be gone by now.  nasr_destroy waits for its
  // streams first, so the event of a destroyed handle has completed: a completed event is dropped here, and a wait is
  // only ever queued on one whose stream still has the work in flight.
  if (hipEventQuery(z.ev_busy) == hipSuccess) {
    z.busy_valid = false;
    return NASR_OK;
  }
  HIPCHK(eh, hipStreamWaitEvent(st, z.ev_busy, 0));
  return NASR_OK;
}

}  // namespace

namespace nasr_impl {

// What a front-end call works out on the host before anything is launched: the resampling plan, every utterance's
// sample and frame offsets.  Errors go to handle eh (the featurizer itself, or the model handle of a batch-slot call).
int fz_plan(nasr_ctx* eh, FzState& z, const std::string& fn, const int64_t* offsets, const int32_t* rates, int n, FzPlan* p) {
  p->rs = false;
  if (rates) {
    std::string why;
    if (!resample_plan(offsets, rates, n, z.cfg.samplerate, &p->rp, &why)) return eh->fail(NASR_ERR_ARG, fn + ": " + why);
    for (const RsUtt& u : p->rp.utt) p->rs = p->rs || u.step != 0;
  }
  p->n = n;
  p->uoff.assign(n + 1, 0);
  p->foff.assign(n + 1, 0);
  for (int i = 0; i < n; ++i) {
    const int64_t len = p->rs ? p->rp.utt[i].n_samples : offsets[i + 1] - offsets[i];
    if (len < 1) return eh->fail(NASR_ERR_ARG, fn + ": utterance " + std::to_string(i) + " has no samples");
    p->uoff[i] = p->rs ? p->rp.utt[i].out_off : offsets[i] - offsets[0];
    p->foff[i + 1] = p->foff[i] + frames_of(z.d.frame_len, z.d.frame_step, len);
  }
  p->S_in = offsets[n] - offsets[0];
  p->uoff[n] = p->rs ? p->rp.total : p->S_in;
  p->mb = (size_t)(n + 1) * 8;
  p->meta_bytes = 2 * p->mb + (size_t)p->foff[n] * 4;
  p->rmeta_bytes = p->rs ? p->rp.utt.size() * sizeof(RsUtt) + p->rp.waves.size() * sizeof(RsWave) : 0;
  return NASR_OK;
}

size_t fz_stage_bytes(const FzPlan& p) {
  return ((size_t)p.S_in * 4 + 7) / 8 * 8 + p.meta_bytes + p.rmeta_bytes + (p.wave ? p.wp.bytes() : 0);
}

// The checks of nasr_wave_aug (include/nasr.h) against the banks, and the kernels' parameters: utterance i's samples are
// [p->uoff[i], p->uoff[i+1]) of the buffer at the featurizer's rate.
int fz_wave_plan(nasr_ctx* eh, FzState& z, const std::string& fn, const nasr_wave_aug* wave, FzPlan* p) {
  p->wave = false;
  if (!wave || (!wave->rir && !wave->noise)) return NASR_OK;
  const int n = p->n;
  const std::string pre = fn + ": waveform augmentation: utterance ";
  p->wp.utt.assign(n, WvUtt{});
  for (int i = 0; i < n; ++i) {
    WvUtt& u = p->wp.utt[i];
    u.off = p->uoff[i];
    u.n = p->uoff[i + 1] - p->uoff[i];
    u.c_len = 1;
    u.noise = -1;
    const int r = wave->rir ? wave->rir[i] : -1, c = wave->noise ? wave->noise[i] : -1;
    const int nr = (int)z.rir_off.size() - 1, ncl = (int)z.noise_off.size() - 1;
    if (r >= 0 || r < -1) {
      if (nr < 1) return eh->fail(NASR_ERR_ARG, pre + std::to_string(i) + " asks for RIR " + std::to_string(r) +
                                                    ", the featurizer has no RIR bank (nasr_featurizer_set_rirs)");
      if (r < 0 || r >= nr)
        return eh->fail(NASR_ERR_ARG, pre + std::to_string(i) + ": RIR index " + std::to_string(r) + " is outside the bank's [0," +
                                          std::to_string(nr - 1) + "] (-1: none)");
      u.h_off = z.rir_off[r];
      u.K = (int32_t)(z.rir_off[r + 1] - z.rir_off[r]);
    }
    if (c >= 0 || c < -1) {
      if (ncl < 1) return eh->fail(NASR_ERR_ARG, pre + std::to_string(i) + " asks for noise clip " + std::to_string(c) +
                                                     ", the featurizer has no noise bank (nasr_featurizer_set_noise)");
      if (c < 0 || c >= ncl)
        return eh->fail(NASR_ERR_ARG, pre + std::to_string(i) + ": noise index " + std::to_string(c) + " is outside the bank's [0," +
                                          std::to_string(ncl - 1) + "] (-1: none)");
      if (!wave->noise_off || !wave->snr_db)
        return eh->fail(NASR_ERR_ARG, pre + std::to_string(i) + " has noise, but noise_off or snr_db is null");
      u.c_off = z.noise_off[c];
      u.c_len = z.noise_off[c + 1] - z.noise_off[c];
      u.c_pos = wave->noise_off[i];
      if (u.c_pos < 0 || u.c_pos >= u.c_len)
        return eh->fail(NASR_ERR_ARG, pre + std::to_string(i) + ": noise_off " + std::to_string(u.c_pos) + " is outside clip " +
                                          std::to_string(c) + "'s [0," + std::to_string(u.c_len - 1) + "]");
      if (!std::isfinite(wave->snr_db[i])) return eh->fail(NASR_ERR_ARG, pre + std::to_string(i) + ": snr_db is not finite");
      u.scale = std::pow(10.0, -(double)wave->snr_db[i] / 20.0);
      u.noise = c;
    }
  }
  wave_tiles(&p->wp);
  p->wave = true;
  return NASR_OK;
}

// The copies, the resampler, mfcc_spectral_kernel and the delta launches of plan p on stream st: z.cep holds the frames
// [F][D] afterwards, z.meta the offsets.  audio: the first utterance's first sample.  pinned (nullable): fz_stage_bytes of pinned memory the
// host-to-device copies go through, so that they are plain DMAs that return at once.
// samples_out (nullable): the call wants the samples at the featurizer's rate, augmented when the plan says so, and no
// features: it returns behind the last kernel that writes them, with ev[2] still to be recorded by the caller.
int fz_front(nasr_ctx* eh, FzState& z, const std::string& fn, const FzPlan& p, const float* audio, void* pinned, hipStream_t st,
             const float** samples_out = nullptr) {
  const int n = p.n;
  const int64_t F = p.foff[n];
  z.hmeta.resize(p.meta_bytes);
  memcpy(z.hmeta.data(), p.uoff.data(), p.mb);
  memcpy(z.hmeta.data() + p.mb, p.foff.data(), p.mb);
  int* fmap = reinterpret_cast<int*>(z.hmeta.data() + 2 * p.mb);
  for (int i = 0; i < n; ++i)
    for (int64_t f = p.foff[i]; f < p.foff[i + 1]; ++f) fmap[f] = i;
  if (int rc = scratch_acquire(eh, z, st)) return rc;
  if (p.rs) {
    if (int rc = resample_prepare(eh, z, p.rp, p.S_in)) return rc;
  }
  const bool feats = !samples_out;
  if (!scratch_ensure(z, z.audio, (size_t)p.S_in * 4) ||
      (feats && (!scratch_ensure(z, z.meta, z.hmeta.size()) || !scratch_ensure(z, z.cep, (size_t)F * z.d.width * 8) ||
                 !scratch_ensure(z, z.mstd, (size_t)n * 16))) ||
      (feats && z.cfg.norm == 1 && (!scratch_ensure(z, z.pfx, (size_t)F * 16) || !scratch_ensure(z, z.fms, (size_t)F * 16))))
    return eh->fail(NASR_ERR_HIP, fn + ": device buffers for " + std::to_string(p.uoff[n]) + " samples could not be allocated");
  const size_t wub = p.wave ? p.wp.utt.size() * sizeof(WvUtt) : 0, wb = p.wave ? p.wp.bytes() : 0;
  if (p.wave) {
    z.hwmeta.resize(wb);
    memcpy(z.hwmeta.data(), p.wp.utt.data(), wub);
    memcpy(z.hwmeta.data() + wub, p.wp.tiles.data(), wb - wub);
    if (!scratch_ensure(z, z.wav, (size_t)p.uoff[n] * 4) || !scratch_ensure(z, z.wmeta, wb) ||
        !scratch_ensure(z, z.wpart, p.wp.tiles.size() * 16) || !scratch_ensure(z, z.gain, (size_t)n * 4))
      return eh->fail(NASR_ERR_HIP, fn + ": device buffers for " + std::to_string(p.uoff[n]) + " augmented samples could not be allocated");
  }
  const void *src_audio = audio, *src_meta = z.hmeta.data(), *src_rmeta = p.rs ? z.hrmeta.data() : nullptr;
  const void* src_wmeta = p.wave ? z.hwmeta.data() : nullptr;
  if (pinned) {
    char* pa = static_cast<char*>(pinned);
    char* pm = pa + ((size_t)p.S_in * 4 + 7) / 8 * 8;
    memcpy(pa, audio, (size_t)p.S_in * 4);
    memcpy(pm, z.hmeta.data(), p.meta_bytes);
    if (p.rs) memcpy(pm + p.meta_bytes, z.hrmeta.data(), p.rmeta_bytes);
    if (p.wave) memcpy(pm + p.meta_bytes + p.rmeta_bytes, z.hwmeta.data(), wb);
    src_audio = pa; src_meta = pm; src_rmeta = pm + p.meta_bytes; src_wmeta = pm + p.meta_bytes + p.rmeta_bytes;
  }
  HIPCHK(eh, hipEventRecord(z.ev[0], st));
  HIPCHK(eh, hipMemcpyAsync(z.audio.p, src_audio, (size_t)p.S_in * 4, hipMemcpyHostToDevice, st));
  if (feats) HIPCHK(eh, hipMemcpyAsync(z.meta.p, src_meta, p.meta_bytes, hipMemcpyHostToDevice, st));
  if (p.rs) HIPCHK(eh, hipMemcpyAsync(z.rmeta.p, src_rmeta, p.rmeta_bytes, hipMemcpyHostToDevice, st));
  if (p.wave) HIPCHK(eh, hipMemcpyAsync(z.wmeta.p, src_wmeta, wb, hipMemcpyHostToDevice, st));
  HIPCHK(eh, hipEventRecord(z.ev[1], st));
  if (p.rs) {
    launch_resample(z.audio.as<float>(), z.rmeta.as<RsUtt>(), rs_waves(z, n), (int64_t)p.rp.waves.size(), z.rs_tab,
                    z.raud.as<float>(), st);
    HIPCHK(eh, hipGetLastError());
  }
  const float* samples = p.rs ? z.raud.as<float>() : z.audio.as<float>();
  if (p.wave) {
    launch_wave_aug(samples, z.wav.as<float>(), z.wmeta.as<WvUtt>(), n, reinterpret_cast<const WvTile*>(z.wmeta.as<char>() + wub),
                    (int64_t)p.wp.tiles.size(), z.rir_bank.as<float>(), z.noise_bank.as<float>(), z.wpart.as<double>(),
                    z.gain.as<float>(), st);
    HIPCHK(eh, hipGetLastError());
    samples = z.wav.as<float>();
  }
  if (samples_out) {
    *samples_out = samples;
    return NASR_OK;
  }
  const int64_t nblk = (F + SPEC_WAVES - 1) / SPEC_WAVES;
  mfcc_spectral_kernel<<<dim3((unsigned)nblk), dim3(64 * SPEC_WAVES), 0, st>>>(
      samples, z.meta.as<int64_t>(), z.meta.as<int64_t>() + (n + 1),
      reinterpret_cast<const int*>(z.meta.as<char>() + 2 * p.mb), nullptr, F, z.tw, z.tw2, z.fb_lo, z.fb_n, z.fb_off, z.fb_w, z.dct,
      z.d, z.cep.as<double>());
  HIPCHK(eh, hipGetLastError());
  const int64_t dblk = (F * z.d.numcep + NORM_THREADS - 1) / NORM_THREADS;
  for (int lv = 1; lv <= z.cfg.deltas; ++lv) {
    mfcc_delta_kernel<<<dim3((unsigned)dblk), dim3(NORM_THREADS), 0, st>>>(
        z.cep.as<double>(), z.meta.as<int64_t>() + (n + 1), reinterpret_cast<const int*>(z.meta.as<char>() + 2 * p.mb), F,
        z.d.numcep, z.d.width, (lv - 1) * z.d.numcep, lv * z.d.numcep);
    HIPCHK(eh, hipGetLastError());
  }
  return NASR_OK;
}

// The device producer of a batch slot's centre frames (nasr_batch.hip slot_fill): the front end of plan p on the slot's
// stream, then mfcc_norm_slot_kernel straight into the slot.  The featurizer's scratch buffers are busy until ev_busy.
int fz_produce_slot(nasr_ctx* eh, nasr_ctx* fzh, const FzPlan& p, const float* audio, int Tb, float* dcentre, float* dpad,
                    void* pinned, hipStream_t st) {
  FzState& z = *fzh->fz;
  const std::string fn = "audio batch";
  int rc = fz_front(eh, z, fn, p, audio, pinned, st);
  if (!rc) {
    if (z.cfg.norm == 1)
      mfcc_causal_slot_kernel<<<dim3(p.n), dim3(NORM_THREADS), 0, st>>>(z.cep.as<double>(), z.meta.as<int64_t>() + (p.n + 1),
                                                                        z.d.width, z.cfg.norm_min_frames, Tb, z.pfx.as<double>(),
                                                                        z.fms.as<double>(), dcentre, dpad);
    else
      mfcc_norm_slot_kernel<<<dim3(p.n), dim3(NORM_THREADS), 0, st>>>(z.cep.as<double>(), z.meta.as<int64_t>() + (p.n + 1),
                                                                      z.d.width, z.d.nc, Tb, dcentre, dpad);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) rc = eh->fail(NASR_ERR_HIP, fn + ": " + hipGetErrorString(e));
  }
  // also when something failed part-way: whatever was queued on st still reads the scratch buffers
  (void)hipEventRecord(z.ev[2], st);
  if (hipEventRecord(z.ev_busy, st) == hipSuccess) z.busy_valid = true;
  z.times_pending = rc == NASR_OK;
  return rc;
}

int fz_feature_width(const nasr_ctx* fzh, int* numcontext, int* frame_width) {
  const FzState& z = *fzh->fz;
  *numcontext = z.d.nc;
  *frame_width = z.d.width;
  return z.W * z.d.width;
}

int fz_static_width(const nasr_ctx* fzh) { return fzh->fz->d.numcep; }

// What a stream session that takes samples keeps (nasr_stream_attach_audio): on the device, per slot, the sample tail
// (capacity frame_len + 1), the running sums, the frames that wait for the M-th, and the ring of the last 2 nc normalised
// frames; on the host the counts that decide what a feed does.  Nothing in it grows with the utterance.
struct FzStream {
  nasr_ctx* fzh = nullptr;             // the featurizer: its tables, and its scratch buffers under the ev_busy protocol
  int S = 0, tail_cap = 0, R = 1;
  DevBuf tail, sums, pend, yring;
  struct Slot {
    int64_t n = 0, nframes = 0, nnorm = 0, rows = 0;   // samples received, frames made, frames normalised, rows emitted
    bool finished = false;
  };
  std::vector<Slot> slot;
};

void FzStreamDelete::operator()(FzStream* f) const { delete f; }

int fz_stream_attach(nasr_ctx* eh, nasr_ctx* fzh, int S, std::unique_ptr<FzStream, FzStreamDelete>* out) {
  const std::string fn = "nasr_stream_attach_audio";
  if (!fzh || !fzh->fz) return eh->fail(NASR_ERR_STATE, fn + ": `featurizer` is not a featurizer handle");
  if (fzh->device != eh->device)
    return eh->fail(NASR_ERR_STATE, fn + ": the model is on device " + std::to_string(eh->device) + ", the featurizer on device " +
                                        std::to_string(fzh->device));
  const FzState& z = *fzh->fz;
  if (z.cfg.norm != 1)
    return eh->fail(NASR_ERR_STATE, fn + ": the featurizer's norm is " + std::to_string(z.cfg.norm) +
                                        ": only the causal normalisation (norm = 1) can be computed while the audio arrives");
  if (z.W * z.d.width != eh->F)
    return eh->fail(NASR_ERR_ARG, fn + ": feature_size " + std::to_string(eh->F) + " must equal (2*numcontext+1)*numcep = (2*" +
                                      std::to_string(z.d.nc) + "+1)*" + std::to_string(z.d.width) + " of the featurizer");
  if (z.d.frame_step > z.d.frame_len)
    return eh->fail(NASR_ERR_ARG, fn + ": frames that leave samples out (winstep > winlen) are not implemented");
  std::unique_ptr<FzStream, FzStreamDelete> a(new FzStream());
  a->fzh = fzh;
  a->S = S;
  a->tail_cap = z.d.frame_len + 1;
  a->R = std::max(1, 2 * z.d.nc);
  a->slot.assign((size_t)S, FzStream::Slot());
  const size_t D = (size_t)z.d.width;
  if (!a->tail.ensure((size_t)S * a->tail_cap * 4, nullptr) || !a->sums.ensure((size_t)S * 16, nullptr) ||
      !a->pend.ensure((size_t)S * z.cfg.norm_min_frames * D * 8, nullptr) || !a->yring.ensure((size_t)S * a->R * D * 4, nullptr))
    return eh->fail(NASR_ERR_HIP, fn + ": hipMalloc of the slots' front-end state failed");
  *out = std::move(a);
  return NASR_OK;
}

void fz_stream_reset(FzStream& a, int slot) {
  // the counts alone: a slot with no frame reads none of its device state
  for (int b = 0; b < a.S; ++b)
    if (slot < 0 || slot == b) a.slot[(size_t)b] = FzStream::Slot();
}

int fz_stream_plan(nasr_ctx* eh, const FzStream& a, const std::string& fn, const int64_t* nnew, const uint8_t* last, FzFeedPlan* p) {
  const FzState& z = *a.fzh->fz;
  const int64_t flen = z.d.frame_len, fstep = z.d.frame_step, M = z.cfg.norm_min_frames, nc = z.d.nc;
  p->slot.assign((size_t)a.S, FzFeedSlot());
  p->seg_total = p->in_total = p->f_total = p->y_total = 0;
  p->Tc = 0;
  for (int b = 0; b < a.S; ++b) {
    const FzStream::Slot& s = a.slot[(size_t)b];
    const bool fin = last && last[b];
    if (nnew[b] < 0) return eh->fail(NASR_ERR_ARG, fn + ": slot " + std::to_string(b) + " has a negative sample count");
    if (s.finished && (nnew[b] > 0 || fin))
      return eh->fail(NASR_ERR_STATE, fn + ": slot " + std::to_string(b) + " holds a finished utterance: nasr_stream_reset it first");
    if (fin && s.n + nnew[b] < 1)
      return eh->fail(NASR_ERR_ARG, fn + ": `last` on slot " + std::to_string(b) + ", which has received no sample");
    FzFeedSlot& d = p->slot[(size_t)b];
    const int64_t n2 = s.n + nnew[b];
    const int64_t full = n2 < flen ? 0 : 1 + (n2 - flen) / fstep;
    const int64_t a0 = std::max<int64_t>(0, s.nframes * fstep - 1);
    d.nfb = s.nframes;
    d.want = s.finished ? s.nframes : fin ? frames_of(flen, fstep, n2) : full;
    d.T = fin ? d.want : -1;
    d.nnorm = s.nnorm;
    d.upto = s.finished ? s.nnorm : (fin || d.want >= M) ? d.want : 0;
    d.rows0 = s.rows;
    d.nrows = (s.finished ? s.rows : fin ? d.want : std::max<int64_t>(0, d.upto - nc)) - s.rows;
    d.ntail = s.finished ? 0 : s.n - a0;
    d.nnew = nnew[b];
    d.lead = s.nframes > 0 ? 1 : 0;
    const int64_t a1 = std::max<int64_t>(0, d.want * fstep - 1);
    d.keep_off = a1 - a0;
    d.nkeep = (fin || s.finished) ? 0 : std::max<int64_t>(0, n2 - a1);
    d.n_after = n2;
    d.seg_off = p->seg_total; d.in_off = p->in_total; d.f_off = p->f_total; d.y_off = p->y_total;
    if (d.nkeep > a.tail_cap || d.ntail > a.tail_cap || d.nrows < 0 || d.upto < d.nnorm || d.want < d.nfb)
      return eh->fail(NASR_ERR_STATE, fn + ": slot " + std::to_string(b) + ": inconsistent front-end state");
    p->seg_total += d.ntail + d.nnew;
    p->in_total += d.nnew;
    p->f_total += d.want - d.nfb;
    p->y_total += d.upto - d.nnorm;
    if (d.nrows > (1 << 24)) return eh->fail(NASR_ERR_ARG, fn + ": slot " + std::to_string(b) + " would emit " + std::to_string(d.nrows) + " rows in one feed");
    p->Tc = std::max(p->Tc, (int)d.nrows);
  }
  if (p->in_total > ((int64_t)1 << 28))
    return eh->fail(NASR_ERR_ARG, fn + ": " + std::to_string(p->in_total) + " samples in one feed: at most 2^28");
  return NASR_OK;
}

void fz_stream_advance(FzStream& a, const FzFeedPlan& p, const uint8_t* last) {
  for (int b = 0; b < a.S; ++b) {
    FzStream::Slot& s = a.slot[(size_t)b];
    const FzFeedSlot& d = p.slot[(size_t)b];
    s.n = d.n_after;
    s.nframes = d.want;
    s.nnorm = d.upto;
    s.rows = d.rows0 + d.nrows;
    s.finished = s.finished || (last && last[b]);
  }
}

int fz_stream_run(nasr_ctx* eh, FzStream& a, const FzFeedPlan& p, const float* audio, float* dfeats, hipStream_t st) {
  FzState& z = *a.fzh->fz;
  const std::string fn = "nasr_stream_feed_audio";
  const int S = a.S, D = z.d.width;
  const int64_t F = p.f_total;
  // the meta block: the slots' descriptors, then what the spectral kernel reads: uoff [S+1], foff [S+1], lead [S], fmap [F]
  const size_t db = (size_t)S * sizeof(FzFeedSlot), ob = (size_t)(S + 1) * 8;
  z.hmeta.resize(db + 2 * ob + (size_t)S * 8 + (size_t)F * 4);
  memcpy(z.hmeta.data(), p.slot.data(), db);
  int64_t* uoff = reinterpret_cast<int64_t*>(z.hmeta.data() + db);
  int64_t* foff = uoff + (S + 1);
  int64_t* lead = foff + (S + 1);
  int* fmap = reinterpret_cast<int*>(lead + S);
  for (int b = 0; b < S; ++b) {
    const FzFeedSlot& d = p.slot[(size_t)b];
    uoff[b] = d.seg_off;
    foff[b] = d.f_off;
    lead[b] = d.lead;
    for (int64_t f = 0; f < d.want - d.nfb; ++f) fmap[d.f_off + f] = b;
  }
  uoff[S] = p.seg_total;
  foff[S] = F;
  int rc = scratch_acquire(eh, z, st);
  if (rc) return rc;
  if (!scratch_ensure(z, z.sin, (size_t)std::max<int64_t>(p.in_total, 1) * 4) ||
      !scratch_ensure(z, z.audio, (size_t)std::max<int64_t>(p.seg_total, 1) * 4) || !scratch_ensure(z, z.meta, z.hmeta.size()) ||
      !scratch_ensure(z, z.cep, (size_t)std::max<int64_t>(F, 1) * D * 8) || !scratch_ensure(z, z.pfx, (size_t)std::max<int64_t>(F, 1) * 16) ||
      !scratch_ensure(z, z.ynew, (size_t)std::max<int64_t>(p.y_total, 1) * D * 4))
    return eh->fail(NASR_ERR_HIP, fn + ": device buffers for " + std::to_string(p.seg_total) + " samples could not be allocated");
  const FzFeedSlot* desc = z.meta.as<FzFeedSlot>();
  const int64_t* d_uoff = reinterpret_cast<const int64_t*>(z.meta.as<char>() + db);
  auto queue = [&]() -> int {
    HIPCHK(eh, hipEventRecord(z.ev[0], st));
    if (p.in_total > 0) HIPCHK(eh, hipMemcpyAsync(z.sin.p, audio, (size_t)p.in_total * 4, hipMemcpyHostToDevice, st));
    HIPCHK(eh, hipMemcpyAsync(z.meta.p, z.hmeta.data(), z.hmeta.size(), hipMemcpyHostToDevice, st));
    HIPCHK(eh, hipEventRecord(z.ev[1], st));
    int64_t longest = 1;
    for (const FzFeedSlot& d : p.slot) longest = std::max(longest, d.ntail + d.nnew);
    const unsigned gx = (unsigned)std::min<int64_t>(64, (longest + NORM_THREADS - 1) / NORM_THREADS);
    mfcc_stream_assemble_kernel<<<dim3(gx, S), dim3(NORM_THREADS), 0, st>>>(desc, a.tail.as<float>(), a.tail_cap,
                                                                             z.sin.as<float>(), z.audio.as<float>());
    HIPCHK(eh, hipGetLastError());
    if (F > 0) {
      const int64_t nblk = (F + SPEC_WAVES - 1) / SPEC_WAVES;
      mfcc_spectral_kernel<<<dim3((unsigned)nblk), dim3(64 * SPEC_WAVES), 0, st>>>(
          z.audio.as<float>(), d_uoff, d_uoff + (S + 1), reinterpret_cast<const int*>(d_uoff + 3 * S + 2), d_uoff + 2 * (S + 1), F,
          z.tw, z.tw2, z.fb_lo, z.fb_n, z.fb_off, z.fb_w, z.dct, z.d, z.cep.as<double>());
      HIPCHK(eh, hipGetLastError());
    }
    mfcc_stream_norm_kernel<<<dim3(S), dim3(NORM_THREADS), 0, st>>>(z.cep.as<double>(), desc, D, z.cfg.norm_min_frames,
                                                                    a.sums.as<double>(), a.pend.as<double>(), z.pfx.as<double>(),
                                                                    z.ynew.as<float>());
    HIPCHK(eh, hipGetLastError());
    if (dfeats) {
      const int64_t ne = (int64_t)S * p.Tc * z.W * D;
      mfcc_stream_stack_kernel<<<dim3((unsigned)((ne + NORM_THREADS - 1) / NORM_THREADS)), dim3(NORM_THREADS), 0, st>>>(
          desc, S, p.Tc, D, z.d.nc, a.R, z.ynew.as<float>(), a.yring.as<float>(), dfeats);
      HIPCHK(eh, hipGetLastError());
    }
    mfcc_stream_carry_kernel<<<dim3(S), dim3(NORM_THREADS), 0, st>>>(desc, D, z.d.nc, a.R, z.ynew.as<float>(), a.yring.as<float>(),
                                                                     z.audio.as<float>(), a.tail.as<float>(), a.tail_cap);
    HIPCHK(eh, hipGetLastError());
    return NASR_OK;
  };
  rc = queue();
  // also when something failed part-way: whatever was queued on st still reads the scratch buffers
  (void)hipEventRecord(z.ev[2], st);
  if (hipEventRecord(z.ev_busy, st) == hipSuccess) z.busy_valid = true;
  z.times_pending = rc == NASR_OK;       // nasr_featurize_times: this feed's copies and front-end kernels
  return rc;
}

}  // namespace nasr_impl

namespace {

// The features of n utterances.  rates == nullptr (nasr_featurize): every utterance is at the config rate.  Otherwise
// an utterance at another rate is resampled to it first, into z.raud, which the MFCC kernels then read.
int featurize(nasr_handle h, const std::string& fn, const float* audio, const int64_t* offsets, const int32_t* rates,
              int n, float* out, int64_t out_rows, double* mean_std) {
  if (!h) return NASR_ERR_ARG;
  FzState* zp = h->fz.get();
  if (!zp) return h->fail(NASR_ERR_STATE, fn + ": not a featurizer handle");
  FzState& z = *zp;
  if (!audio || !offsets || !out || n < 1) return h->fail(NASR_ERR_ARG, fn + ": null buffer or n < 1");
  FzPlan p;
  if (int rc = fz_plan(h, z, fn, offsets, rates, n, &p)) return rc;
  const int64_t F = p.foff[n];
  if (out_rows != F)
    return h->fail(NASR_ERR_ARG, fn + ": out_rows is " + std::to_string(out_rows) + ", the utterances have " +
                                     std::to_string(F) + " frames");
  const size_t rowlen = (size_t)z.W * z.d.width;
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = scratch_acquire(h, z, h->st)) return rc;
  if (!z.out.ensure((size_t)F * rowlen * 4, nullptr))
    return h->fail(NASR_ERR_HIP, fn + ": device buffers for " + std::to_string(p.uoff[n]) + " samples could not be allocated");
  if (int rc = fz_front(h, z, fn, p, audio + offsets[0], nullptr, h->st)) return rc;
  if (z.cfg.norm == 1)
    mfcc_causal_norm_kernel<<<dim3(n), dim3(NORM_THREADS), 0, h->st>>>(z.cep.as<double>(), z.meta.as<int64_t>() + (n + 1),
                                                                      z.d.width, z.d.nc, z.cfg.norm_min_frames,
                                                                      z.pfx.as<double>(), z.fms.as<double>(),
                                                                      z.out.as<float>(), z.mstd.as<double>());
  else
    mfcc_norm_kernel<<<dim3(n), dim3(NORM_THREADS), 0, h->st>>>(z.cep.as<double>(), z.meta.as<int64_t>() + (n + 1), z.d.width,
                                                               z.d.nc, z.out.as<float>(), z.mstd.as<double>());
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(z.ev[2], h->st));
  HIPCHK(h, hipMemcpyAsync(out, z.out.p, (size_t)F * rowlen * 4, hipMemcpyDeviceToHost, h->st));
  if (mean_std) HIPCHK(h, hipMemcpyAsync(mean_std, z.mstd.p, (size_t)n * 16, hipMemcpyDeviceToHost, h->st));
  HIPCHK(h, hipEventRecord(z.ev[3], h->st));
  return finish(h, z);
}

}  // namespace

extern "C" {

int64_t nasr_mfcc_frames(const nasr_mfcc_cfg* cfg, int64_t num_samples) {
  std::string why;
  if (!cfg_ok(cfg, &why) || num_samples < 1) return NASR_ERR_ARG;
  return frames_of(round_half_up(cfg->winlen * cfg->samplerate), std::max<int64_t>(1, round_half_up(cfg->winstep * cfg->samplerate)),
                   num_samples);
}

int nasr_mfcc_width(const nasr_mfcc_cfg* cfg) {
  std::string why;
  if (!cfg_ok(cfg, &why)) return NASR_ERR_ARG;
  return cfg->numcep * (1 + cfg->deltas);
}

int nasr_mfcc_filterbank(const nasr_mfcc_cfg* cfg, int32_t* bins, float* weights) {
  std::string why;
  if (!cfg_ok(cfg, &why)) return NASR_ERR_ARG;
  const std::vector<double> bin = filter_bins(cfg);
  if (bins)
    for (size_t i = 0; i < bin.size(); ++i) bins[i] = (int32_t)bin[i];
  if (weights) {
    const std::vector<double> w = filter_weights(cfg, bin);
    for (size_t i = 0; i < w.size(); ++i) weights[i] = (float)w[i];
  }
  return NASR_OK;
}

int nasr_create_featurizer(const nasr_mfcc_cfg* cfg, int device_id, void* stream, nasr_handle* out) {
  if (!cfg || !out) {
    g_create_error = "nasr_create_featurizer: null argument";
    return NASR_ERR_ARG;
  }
  *out = nullptr;
  std::string why;
  if (!cfg_ok(cfg, &why)) {
    g_create_error = "nasr_create_featurizer: " + why;
    return NASR_ERR_ARG;
  }
  const int64_t flen = round_half_up(cfg->winlen * cfg->samplerate), fstep = round_half_up(cfg->winstep * cfg->samplerate);
  if (flen < 1 || fstep < 1 || flen > (1 << 30) || fstep > (1 << 30)) {
    g_create_error = "nasr_create_featurizer: winlen * samplerate and winstep * samplerate must round to >= 1 sample";
    return NASR_ERR_ARG;
  }
  nasr_ctx* h = nullptr;
  if (int rc = handle_open("nasr_create_featurizer", Family::Featurizer, device_id, stream, &h, nullptr)) return rc;
  h->graph_mode = false;
  h->fz.reset(new FzState());
  FzState& z = *h->fz;
  z.cfg = *cfg;
  z.d = FzDims{(int)flen, (int)fstep, cfg->numcep, cfg->nfilt, cfg->numcontext, cfg->append_energy ? 1 : 0, cfg->preemph,
                 cfg->kind, cfg->numcep * (1 + cfg->deltas)};
  z.W = 2 * cfg->numcontext + 1;
  for (Event& e : z.ev)
    if (hipEventCreate(e.out()) != hipSuccess) return create_fail(h, NASR_ERR_HIP, "hipEventCreate failed");
  if (hipEventCreateWithFlags(z.ev_busy.out(), hipEventDisableTiming) != hipSuccess)
    return create_fail(h, NASR_ERR_HIP, "hipEventCreate failed");

  const double pi = 3.14159265358979323846;
  std::vector<double2> tw(FFT_N), tw2(NBIN);
  for (int t = 0; t < FFT_N; ++t) tw[t] = make_double2(std::cos(-2 * pi * t / FFT_N), std::sin(-2 * pi * t / FFT_N));
  for (int k = 0; k < NBIN; ++k) tw2[k] = make_double2(std::cos(-pi * k / FFT_N), std::sin(-pi * k / FFT_N));
  // the filters as (first bin, count, weights): each filter's span [bin[j], bin[j+2]) of the dense table
  const int nf = cfg->nfilt, nc = cfg->numcep;
  const std::vector<double> bin = filter_bins(cfg);
  const std::vector<double> wd = filter_weights(cfg, bin);
  std::vector<int> lo(nf), cnt(nf), off(nf);
  std::vector<double> w;
  for (int j = 0; j < nf; ++j) {
    const int a = std::max(0, (int)bin[j]), b = std::min(NBIN, std::max(a, (int)bin[j + 2]));
    lo[j] = a;
    cnt[j] = b - a;
    off[j] = (int)w.size();
    for (int i = a; i < b; ++i) w.push_back(wd[(size_t)j * NBIN + i]);
  }
  if (w.empty()) w.push_back(0.0);
  // DCT-II, norm='ortho', times the lifter 1 + (L/2) sin(pi n / L): dct[j][n]
  std::vector<double> dct((size_t)nf * nc);
  for (int n = 0; n < nc; ++n) {
    const double sc = n == 0 ? std::sqrt(1.0 / nf) : std::sqrt(2.0 / nf);
    const double lift = cfg->ceplifter > 0 ? 1.0 + 0.5 * cfg->ceplifter * std::sin(pi * n / cfg->ceplifter) : 1.0;
    for (int j = 0; j < nf; ++j) dct[(size_t)j * nc + n] = sc * lift * std::cos(pi * n * (2 * j + 1) / (2.0 * nf));
  }
  auto put = [&](auto& dst, const auto& v) {
    using T = typename std::decay_t<decltype(v)>::value_type;
    if (hipMalloc(dst.out(), v.size() * sizeof(T)) != hipSuccess) return false;
    return hipMemcpy(dst.get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
  };
  if (!put(z.tw, tw) || !put(z.tw2, tw2) || !put(z.fb_lo, lo) || !put(z.fb_n, cnt) || !put(z.fb_off, off) ||
      !put(z.fb_w, w) || !put(z.dct, dct))
    return create_fail(h, NASR_ERR_HIP, "nasr_create_featurizer: upload of the tables failed");
  *out = h;
  return NASR_OK;
}

int nasr_featurize(nasr_handle h, const float* audio, const int64_t* offsets, int n, float* out, int64_t out_rows,
                   double* mean_std) {
  return featurize(h, "nasr_featurize", audio, offsets, nullptr, n, out, out_rows, mean_std);
}

int nasr_featurize_rates(nasr_handle h, const float* audio, const int64_t* offsets, const int32_t* rates, int n,
                         float* out, int64_t out_rows, double* mean_std) {
  if (h && h->fz && !rates) return h->fail(NASR_ERR_ARG, "nasr_featurize_rates: null rates");
  return featurize(h, "nasr_featurize_rates", audio, offsets, rates, n, out, out_rows, mean_std);
}

int nasr_resample(nasr_handle h, const float* audio, const int64_t* offsets, const int32_t* rates, int n, float* out,
                  int64_t out_len) {
  if (!h) return NASR_ERR_ARG;
  FzState* zp = h->fz.get();
  if (!zp) return h->fail(NASR_ERR_STATE, "nasr_resample: not a featurizer handle");
  FzState& z = *zp;
  if (!audio || !offsets || !rates || !out || n < 1) return h->fail(NASR_ERR_ARG, "nasr_resample: null buffer or n < 1");
  ResamplePlan plan;
  std::string why;
  if (!resample_plan(offsets, rates, n, z.cfg.samplerate, &plan, &why)) return h->fail(NASR_ERR_ARG, "nasr_resample: " + why);
  if (out_len != plan.total)
    return h->fail(NASR_ERR_ARG, "nasr_resample: out_len is " + std::to_string(out_len) + ", the utterances resample to " +
                                     std::to_string(plan.total) + " samples");
  const int64_t S = offsets[n] - offsets[0];
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = scratch_acquire(h, z, h->st)) return rc;
  if (int rc = resample_prepare(h, z, plan, S)) return rc;
  HIPCHK(h, hipEventRecord(z.ev[0], h->st));
  HIPCHK(h, hipMemcpyAsync(z.audio.p, audio + offsets[0], (size_t)S * 4, hipMemcpyHostToDevice, h->st));
  HIPCHK(h, hipMemcpyAsync(z.rmeta.p, z.hrmeta.data(), z.hrmeta.size(), hipMemcpyHostToDevice, h->st));
  HIPCHK(h, hipEventRecord(z.ev[1], h->st));
  launch_resample(z.audio.as<float>(), z.rmeta.as<RsUtt>(), rs_waves(z, n), (int64_t)plan.waves.size(), z.rs_tab,
                  z.raud.as<float>(), h->st);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(z.ev[2], h->st));
  HIPCHK(h, hipMemcpyAsync(out, z.raud.p, (size_t)plan.total * 4, hipMemcpyDeviceToHost, h->st));
  HIPCHK(h, hipEventRecord(z.ev[3], h->st));
  return finish(h, z);
}

int nasr_augment_audio(nasr_handle h, const float* audio, const int64_t* offsets, const int32_t* rates, int n,
                       const nasr_wave_aug* wave, float* out, int64_t out_len) {
  const std::string fn = "nasr_augment_audio";
  if (!h) return NASR_ERR_ARG;
  FzState* zp = h->fz.get();
  if (!zp) return h->fail(NASR_ERR_STATE, fn + ": not a featurizer handle");
  FzState& z = *zp;
  if (!audio || !offsets || !out || n < 1) return h->fail(NASR_ERR_ARG, fn + ": null buffer or n < 1");
  FzPlan p;
  if (int rc = fz_plan(h, z, fn, offsets, rates, n, &p)) return rc;
  if (int rc = fz_wave_plan(h, z, fn, wave, &p)) return rc;
  if (out_len != p.uoff[n])
    return h->fail(NASR_ERR_ARG, fn + ": out_len is " + std::to_string(out_len) + ", the utterances have " + std::to_string(p.uoff[n]) +
                                     " samples at the featurizer's rate");
  HIPCHK(h, hipSetDevice(h->device));
  const float* samples = nullptr;
  if (int rc = fz_front(h, z, fn, p, audio + offsets[0], nullptr, h->st, &samples)) return rc;
  HIPCHK(h, hipEventRecord(z.ev[2], h->st));
  HIPCHK(h, hipMemcpyAsync(out, samples, (size_t)out_len * 4, hipMemcpyDeviceToHost, h->st));
  HIPCHK(h, hipEventRecord(z.ev[3], h->st));
  return finish(h, z);
}

// A bank of the featurizer (noise clips, RIRs): the checks, then the upload; `what` names an entry in the messages.
static int set_bank(nasr_ctx* h, const std::string& fn, const char* what, const float* data, const int64_t* offsets, int n,
                    int64_t max_len, DevBuf FzState::*bank, std::vector<int64_t> FzState::*off) {
  if (!h) return NASR_ERR_ARG;
  FzState* zp = h->fz.get();
  if (!zp) return h->fail(NASR_ERR_STATE, fn + ": not a featurizer handle");
  FzState& z = *zp;
  if (n < 0 || (n > 0 && (!data || !offsets))) return h->fail(NASR_ERR_ARG, fn + ": null buffer or a negative count");
  std::vector<int64_t> o(n > 0 ? n + 1 : 0, 0);
  for (int i = 0; i < n; ++i) {
    const int64_t len = offsets[i + 1] - offsets[i];
    if (offsets[0] < 0 || len < 1) return h->fail(NASR_ERR_ARG, fn + ": " + what + " " + std::to_string(i) + " is empty");
    if (max_len > 0 && len > max_len)
      return h->fail(NASR_ERR_ARG, fn + ": " + what + " " + std::to_string(i) + " has " + std::to_string(len) + " taps, at most " +
                                       std::to_string(max_len) + " (NASR_AUG_MAX_RIR_TAPS) are taken");
    for (int64_t k = offsets[i]; k < offsets[i + 1]; ++k)
      if (!std::isfinite(data[k]))
        return h->fail(NASR_ERR_ARG, fn + ": " + what + " " + std::to_string(i) + " holds a value that is not finite (at " +
                                         std::to_string(k - offsets[i]) + ")");
    o[i + 1] = offsets[i + 1] - offsets[0];
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (z.busy_valid) {                    // a batch-slot call may still read the old bank on a model's stream
    (void)hipEventSynchronize(z.ev_busy);
    z.busy_valid = false;
  }
  (z.*bank).release();
  (z.*off).clear();
  if (n == 0) return NASR_OK;
  const size_t bytes = (size_t)o[n] * 4;
  if (!(z.*bank).ensure(bytes, nullptr)) return h->fail(NASR_ERR_HIP, fn + ": the bank's " + std::to_string(bytes) + " bytes could not be allocated");
  HIPCHK(h, hipMemcpy((z.*bank).p, data + offsets[0], bytes, hipMemcpyHostToDevice));
  (z.*off) = std::move(o);
  return NASR_OK;
}

int nasr_featurizer_set_noise(nasr_handle h, const float* samples, const int64_t* offsets, int n_clips) {
  return set_bank(h, __func__, "noise clip", samples, offsets, n_clips, 0, &FzState::noise_bank, &FzState::noise_off);
}

int nasr_featurizer_set_rirs(nasr_handle h, const float* taps, const int64_t* offsets, int n_rirs) {
  return set_bank(h, __func__, "RIR", taps, offsets, n_rirs, WV_MAX_TAPS, &FzState::rir_bank, &FzState::rir_off);
}

int nasr_featurize_times(nasr_handle h, float* h2d_ms, float* kernel_ms, float* d2h_ms) {
  if (!h) return NASR_ERR_ARG;
  if (!h->fz) return h->fail(NASR_ERR_STATE, "nasr_featurize_times: not a featurizer handle");
  if (h->fz->times_pending) {           // a batch-slot call: copies and kernels on the model's stream, nothing comes back
    FzState& z = *h->fz;
    HIPCHK(h, hipEventSynchronize(z.ev[2]));
    for (int i = 0; i < 2; ++i)
      if (hipEventElapsedTime(&z.times[i], z.ev[i], z.ev[i + 1]) != hipSuccess) z.times[i] = 0.f;
    z.times[2] = 0.f;
    z.times_pending = false;
  }
  if (h2d_ms) *h2d_ms = h->fz->times[0];
  if (kernel_ms) *kernel_ms = h->fz->times[1];
  if (d2h_ms) *d2h_ms = h->fz->times[2];
  return NASR_OK;
}

}  // extern "C"
