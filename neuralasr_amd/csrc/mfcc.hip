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
// Tables (twiddles, filter weights, the DCT x lifter matrix) are built once per handle on the host in double.
// nasr_featurize_rates first resamples utterances at other rates to the config rate (resample.hip) into a device
// buffer, which the same two kernels then read.
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
__global__ __launch_bounds__(64 * SPEC_WAVES) void mfcc_spectral_kernel(
    const float* __restrict__ audio, const int64_t* __restrict__ uoff, const int64_t* __restrict__ foff,
    const int* __restrict__ fmap, int64_t nframes, const double2* __restrict__ tw, const double2* __restrict__ tw2,
    const int* __restrict__ fb_lo, const int* __restrict__ fb_n, const int* __restrict__ fb_off,
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
    t0 = (f - foff[u]) * (int64_t)d.frame_step;
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
  std::vector<char> hmeta;
  DevPtr<double2> rs_tab;              // the resampling filter's (table[k], table[k+1]) pairs, made at the first use
  DevBuf raud, rmeta;                  // resampled audio; the resampling plan (RsUtt [n], then RsWave [waves])
  std::vector<char> hrmeta;
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

size_t fz_stage_bytes(const FzPlan& p) { return ((size_t)p.S_in * 4 + 7) / 8 * 8 + p.meta_bytes + p.rmeta_bytes; }

// The copies, the resampler, mfcc_spectral_kernel and the delta launches of plan p on stream st: z.cep holds the frames
// [F][D] afterwards, z.meta the offsets.  audio: the first utterance's first sample.  pinned (nullable): fz_stage_bytes of pinned memory the
// host-to-device copies go through, so that they are plain DMAs that return at once.
int fz_front(nasr_ctx* eh, FzState& z, const std::string& fn, const FzPlan& p, const float* audio, void* pinned, hipStream_t st) {
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
  if (!scratch_ensure(z, z.audio, (size_t)p.S_in * 4) || !scratch_ensure(z, z.meta, z.hmeta.size()) ||
      !scratch_ensure(z, z.cep, (size_t)F * z.d.width * 8) || !scratch_ensure(z, z.mstd, (size_t)n * 16))
    return eh->fail(NASR_ERR_HIP, fn + ": device buffers for " + std::to_string(p.uoff[n]) + " samples could not be allocated");
  const void *src_audio = audio, *src_meta = z.hmeta.data(), *src_rmeta = p.rs ? z.hrmeta.data() : nullptr;
  if (pinned) {
    char* pa = static_cast<char*>(pinned);
    char* pm = pa + ((size_t)p.S_in * 4 + 7) / 8 * 8;
    memcpy(pa, audio, (size_t)p.S_in * 4);
    memcpy(pm, z.hmeta.data(), p.meta_bytes);
    if (p.rs) memcpy(pm + p.meta_bytes, z.hrmeta.data(), p.rmeta_bytes);
    src_audio = pa; src_meta = pm; src_rmeta = pm + p.meta_bytes;
  }
  HIPCHK(eh, hipEventRecord(z.ev[0], st));
  HIPCHK(eh, hipMemcpyAsync(z.audio.p, src_audio, (size_t)p.S_in * 4, hipMemcpyHostToDevice, st));
  HIPCHK(eh, hipMemcpyAsync(z.meta.p, src_meta, p.meta_bytes, hipMemcpyHostToDevice, st));
  if (p.rs) HIPCHK(eh, hipMemcpyAsync(z.rmeta.p, src_rmeta, p.rmeta_bytes, hipMemcpyHostToDevice, st));
  HIPCHK(eh, hipEventRecord(z.ev[1], st));
  if (p.rs) {
    launch_resample(z.audio.as<float>(), z.rmeta.as<RsUtt>(), rs_waves(z, n), (int64_t)p.rp.waves.size(), z.rs_tab,
                    z.raud.as<float>(), st);
    HIPCHK(eh, hipGetLastError());
  }
  const int64_t nblk = (F + SPEC_WAVES - 1) / SPEC_WAVES;
  mfcc_spectral_kernel<<<dim3((unsigned)nblk), dim3(64 * SPEC_WAVES), 0, st>>>(
      p.rs ? z.raud.as<float>() : z.audio.as<float>(), z.meta.as<int64_t>(), z.meta.as<int64_t>() + (n + 1),
      reinterpret_cast<const int*>(z.meta.as<char>() + 2 * p.mb), F, z.tw, z.tw2, z.fb_lo, z.fb_n, z.fb_off, z.fb_w, z.dct,
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
