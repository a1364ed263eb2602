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
//   mfcc_norm_kernel<RULE, FORM>
//                         one workgroup per utterance, the statistics of RULE written in the layout of FORM.
//                         RULE 0, the whole-utterance rule: the float64 mean and std of the stacked matrix from the centre
//                         frames (each counted once per window that holds it, the zero pads as a count).  RULE 1, the
//                         causal rule (cfg.norm = 1; the reference has no causal front end): the per-frame
//                         sums p1, p2 in parallel over frames, their prefix sums S1, S2 by ONE lane each in frame order,
//                         then frame u normalised with the statistics of its first n_u = min(T, max(u+1, M)) frames;
//                         context frames outside the utterance are exact zeros.  FORM 0: the normalised rows written
//                         straight into the stacked layout.  FORM 1, as a model handle's batch slot takes them
//                         (nasr_batch.hip): the normalised centre frames [B][T][D] of a whole batch, zeros past each
//                         utterance's end, and one out-of-utterance value per utterance; nasr_upload_batch_audio
//   mfcc_stream_*_kernel  a stream session that takes samples (nasr_stream_feed_audio): per slot the carried sample tail and
//                         the new samples become one segment (assemble), mfcc_spectral_kernel runs on the newly complete
//                         frames, the prefix continues from the carried sums and the frames that have become normalisable
//                         are normalised (norm), the chunk's stacked rows go straight into the batch slot (stack), and the
//                         ring of the last 2 nc normalised frames and the tail are left for the next feed (carry)
// Tables (twiddles, filter weights, the DCT x lifter matrix) are built once per handle on the host in double
// (fz_host_tables).  The kernels stay in this file: a host caller goes through the launchers of mfcc.h, and the
// featurizer handle that owns the buffers and orders the launches is nasr_fz.hip.
#include "mfcc.h"

#include <algorithm>
#include <cmath>

using namespace nasr_impl;

namespace {

constexpr int FFT_N = 256;              // complex points: nfft = 512 real samples
constexpr int NBIN = 257;               // nfft/2 + 1
constexpr int MAX_FILT = 128;
constexpr int SPEC_WAVES = 4;           // frames per workgroup
constexpr int NORM_THREADS = 256;
constexpr double F64_EPS = 2.220446049250313e-16;   // numpy.finfo(float).eps: psf's stand-in for exact zeros

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
// `numcep` here is the width of a frame of the cep buffer: D = numcep (1 + deltas).
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

// ------------------------------------------------------------------------------------------- the normalise kernel
// One workgroup per utterance u of T frames [T][D] at src.  The rule runs first and leaves the writers two things: stat(t),
// the (mean, sd) that frame t is normalised with, and `outside`, the value of a context frame outside the utterance.
//   RULE 0, the whole utterance: one pair (utt_mean_std) for every frame; outside = norm_value(0, mean, sd).
//   RULE 1, causal: frame t's pair is ms[t] (causal_utt_stats; pfx and ms are [F][2] scratch, indexed like the frames),
//           stat(T-1) is that of all T frames; outside is an exact 0.
// Each writer is written once over them, every element through norm_value.
//   FORM 0, stacked: out[t][w*D + c] = y[t+w-nc][c], `outside` where t+w-nc is no frame of the utterance, utterance after
//           utterance; mstd (nullable) gets (mean, sd) of all T frames.
//   FORM 1, the batch slot (the `centre` layout of nasr_upload_batch_context): out [B][Tb][D] gets utterance u's normalised
//           frames and exact zeros for t >= T, pad[u] gets `outside`.  Consecutive threads write consecutive floats.
// The arguments that every instantiation reads stand together in front: an argument between ones that an instantiation
// does not read is loaded on its own, late, and a lone load of the argument segment cost the slot form 1.3 us.
template <int RULE, int FORM>
__global__ __launch_bounds__(NORM_THREADS) void mfcc_norm_kernel(const double* __restrict__ cep,
                                                                 const int64_t* __restrict__ foff, int D, int nc, int Tb,
                                                                 int M, float* __restrict__ out, float* __restrict__ pad,
                                                                 double* __restrict__ mstd, double* pfx, double* ms) {
  __shared__ double sh[RULE == 0 ? 1 : 2][NORM_THREADS];
  const int u = blockIdx.x, tid = threadIdx.x;
  const int64_t f0 = foff[u], T = foff[u + 1] - f0;
  const double* src = cep + f0 * D;
  const double* m = RULE == 0 ? nullptr : ms + 2 * f0;
  double mean = 0.0, sd = 1.0;
  if (RULE == 0) utt_mean_std(src, T, D, nc, sh[0], &mean, &sd);
  else causal_utt_stats(src, T, D, M, pfx + 2 * f0, ms + 2 * f0, sh);
  auto stat = [&](int64_t t, double* a, double* b) {
    *a = RULE == 0 ? mean : m[2 * t];
    *b = RULE == 0 ? sd : m[2 * t + 1];
  };
  auto y = [&](int64_t i, int64_t t) {    // element i of the utterance's frames, which is frame t's
    double a, b;
    stat(t, &a, &b);
    return norm_value(src[i], a, b);
  };
  const float outside = RULE == 0 ? norm_value(0.0, mean, sd) : 0.f;
  if (FORM == 0) {
    if (mstd && tid == 0) stat(T - 1, &mstd[2 * u], &mstd[2 * u + 1]);
    const int rowlen = (2 * nc + 1) * D;
    float* dst = out + f0 * rowlen;
    for (int64_t e = tid; e < T * rowlen; e += NORM_THREADS) {
      const int64_t t = e / rowlen;
      const int r = (int)(e - t * rowlen);
      const int64_t ts = t + r / D - nc;
      dst[e] = (ts >= 0 && ts < T) ? y(ts * D + r % D, ts) : outside;
    }
  } else {
    if (tid == 0) pad[u] = outside;
    const int64_t ne = T * D, nb = (int64_t)Tb * D;
    float* dst = out + (int64_t)u * nb;
    for (int64_t e = tid; e < nb; e += NORM_THREADS) dst[e] = e < ne ? y(e, e / D) : 0.f;
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

}  // namespace

namespace nasr_impl {

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

FzHostTables fz_host_tables(const nasr_mfcc_cfg* cfg) {
  FzHostTables t;
  const double pi = 3.14159265358979323846;
  t.tw.resize(FFT_N);
  t.tw2.resize(NBIN);
  for (int k = 0; k < FFT_N; ++k) t.tw[k] = make_double2(std::cos(-2 * pi * k / FFT_N), std::sin(-2 * pi * k / FFT_N));
  for (int k = 0; k < NBIN; ++k) t.tw2[k] = make_double2(std::cos(-pi * k / FFT_N), std::sin(-pi * k / FFT_N));
  // the filters as (first bin, count, weights): each filter's span [bin[j], bin[j+2]) of the dense table
  const int nf = cfg->nfilt, nc = cfg->numcep;
  const std::vector<double> bin = filter_bins(cfg);
  const std::vector<double> wd = filter_weights(cfg, bin);
  t.fb_lo.resize(nf);
  t.fb_n.resize(nf);
  t.fb_off.resize(nf);
  for (int j = 0; j < nf; ++j) {
    const int a = std::max(0, (int)bin[j]), b = std::min(NBIN, std::max(a, (int)bin[j + 2]));
    t.fb_lo[j] = a;
    t.fb_n[j] = b - a;
    t.fb_off[j] = (int)t.fb_w.size();
    for (int i = a; i < b; ++i) t.fb_w.push_back(wd[(size_t)j * NBIN + i]);
  }
  if (t.fb_w.empty()) t.fb_w.push_back(0.0);
  // DCT-II, norm='ortho', times the lifter 1 + (L/2) sin(pi n / L): dct[j][n]
  t.dct.resize((size_t)nf * nc);
  for (int n = 0; n < nc; ++n) {
    const double sc = n == 0 ? std::sqrt(1.0 / nf) : std::sqrt(2.0 / nf);
    const double lift = cfg->ceplifter > 0 ? 1.0 + 0.5 * cfg->ceplifter * std::sin(pi * n / cfg->ceplifter) : 1.0;
    for (int j = 0; j < nf; ++j) t.dct[(size_t)j * nc + n] = sc * lift * std::cos(pi * n * (2 * j + 1) / (2.0 * nf));
  }
  return t;
}

// ------------------------------------------------------------------------------------------------------ launchers
void launch_mfcc_spectral(const float* audio, const int64_t* uoff, const int64_t* foff, const int* fmap, const int64_t* ulead,
                          int64_t nframes, const FzTables& t, const FzDims& d, double* cep, hipStream_t st) {
  const int64_t nblk = (nframes + SPEC_WAVES - 1) / SPEC_WAVES;
  mfcc_spectral_kernel<<<dim3((unsigned)nblk), dim3(64 * SPEC_WAVES), 0, st>>>(audio, uoff, foff, fmap, ulead, nframes, t.tw, t.tw2,
                                                                               t.fb_lo, t.fb_n, t.fb_off, t.fb_w, t.dct, d, cep);
}

void launch_mfcc_delta(double* cep, const int64_t* foff, const int* fmap, int64_t nframes, int numcep, int width, int src, int dst,
                       hipStream_t st) {
  const int64_t nblk = (nframes * numcep + NORM_THREADS - 1) / NORM_THREADS;
  mfcc_delta_kernel<<<dim3((unsigned)nblk), dim3(NORM_THREADS), 0, st>>>(cep, foff, fmap, nframes, numcep, width, src, dst);
}

void launch_mfcc_norm(const double* cep, const int64_t* foff, int n, int D, int nc, int rule, int M, double* pfx, double* ms,
                      bool slot, int Tb, float* out, float* pad, double* mstd, hipStream_t st) {
  auto kernel = rule == 1 ? (slot ? mfcc_norm_kernel<1, 1> : mfcc_norm_kernel<1, 0>)
                          : (slot ? mfcc_norm_kernel<0, 1> : mfcc_norm_kernel<0, 0>);
  kernel<<<dim3(n), dim3(NORM_THREADS), 0, st>>>(cep, foff, D, nc, Tb, M, out, pad, mstd, pfx, ms);
}

void launch_mfcc_stream_assemble(const FzFeedSlot* desc, int S, int64_t longest, const float* tail, int tail_cap, const float* in,
                                 float* seg, hipStream_t st) {
  const unsigned gx = (unsigned)std::min<int64_t>(64, (longest + NORM_THREADS - 1) / NORM_THREADS);
  mfcc_stream_assemble_kernel<<<dim3(gx, S), dim3(NORM_THREADS), 0, st>>>(desc, tail, tail_cap, in, seg);
}

void launch_mfcc_stream_norm(const double* cep, const FzFeedSlot* desc, int S, int D, int M, double* sums, double* pend,
                             double* pfx, float* ynew, hipStream_t st) {
  mfcc_stream_norm_kernel<<<dim3(S), dim3(NORM_THREADS), 0, st>>>(cep, desc, D, M, sums, pend, pfx, ynew);
}

void launch_mfcc_stream_stack(const FzFeedSlot* desc, int S, int Tc, int D, int nc, int R, const float* ynew, const float* yring,
                              float* out, hipStream_t st) {
  const int64_t ne = (int64_t)S * Tc * (2 * nc + 1) * D;
  mfcc_stream_stack_kernel<<<dim3((unsigned)((ne + NORM_THREADS - 1) / NORM_THREADS)), dim3(NORM_THREADS), 0, st>>>(
      desc, S, Tc, D, nc, R, ynew, yring, out);
}

void launch_mfcc_stream_carry(const FzFeedSlot* desc, int S, int D, int nc, int R, const float* ynew, float* yring,
                              const float* seg, float* tail, int tail_cap, hipStream_t st) {
  mfcc_stream_carry_kernel<<<dim3(S), dim3(NORM_THREADS), 0, st>>>(desc, D, nc, R, ynew, yring, seg, tail, tail_cap);
}

}  // namespace nasr_impl

