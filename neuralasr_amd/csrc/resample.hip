// resample.hip — librosa.load's resampling to the config rate (reference utils.py:25), librosa 0.6-0.9 with
// res_type='kaiser_best' (resampy 0.2), on the GPU: the native audio is uploaded once and the resampled samples are
// written into the buffer the MFCC kernels read (mfcc.hip).
//   resample_kernel  one lane per output sample, several utterances (each at its own rate) per launch.  resampy's
//                    resample_f restated tap for tap in float64 with no contraction: the left wing (i = 0..) then the
//                    right wing (k = 0..), each weight table[j] + eta * delta[j], and the float32 sum rounded after
//                    every tap (resampy's y is float32: y = float32(double(y) + w * double(x))).
// The time register is resampy's sequential `tr += 1 / ratio` in float64: exact rational positions differ from it
// where a position crosses an integer, so the host runs the same loop and records the register at the
// start of every 64 outputs; lane j of a wave continues it with j more adds, the same additions in the same order.
// The table (32769 float64, 256 KiB) is read as (table[k], table[k+1]) pairs through the vector caches: for a fixed
// tap every lane of a wave reads within one `step`-wide window (<= 4 KiB of pairs), so the L1 serves it.  When
// ratio < 1 resampy scales the table by ratio before np.diff; the kernel scales both entries of a pair and subtracts,
// which is that diff bit for bit (and the scale is 1.0, exact, when ratio >= 1).
#include "nasr_ctx.h"
#include "resample.h"

#include <cmath>

using namespace nasr;
using namespace nasr_impl;

namespace {

constexpr int RS_THREADS = 256;
constexpr double RS_ROLLOFF = 0.9475937167399596;   // kaiser_best
constexpr double RS_BETA = 14.769656459379492;

__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const float* __restrict__ x, const RsUtt* __restrict__ utt,
                                                              const RsWave* __restrict__ waves, int64_t nwaves,
                                                              const double2* __restrict__ tab, float* __restrict__ y) {
#pragma clang fp contract(off)
  const int64_t w = (int64_t)blockIdx.x * (RS_THREADS / 64) + (threadIdx.x >> 6);
  if (w >= nwaves) return;
  const int lane = threadIdx.x & 63;
  const RsWave wv = waves[w];
  const RsUtt u = utt[wv.u];
  const int64_t t = wv.t0 + lane;
  if (t >= u.n_samples) return;
  const float* xs = x + u.in_off;
  float acc = 0.f;
  if (u.step == 0) {
    acc = xs[t];
  } else if (t < u.n_out) {
    double tr = wv.tr0;
    for (int j = 0; j < lane; ++j) tr += u.inc;
    const int64_t n = (int64_t)tr;
    double frac = u.scale * (tr - (double)n);
    double idx = frac * RS_TABLE;
    int off = (int)idx;
    double eta = idx - off;
    const int64_t imax = min(n + 1, (int64_t)((RS_NWIN - off) / u.step));
    for (int64_t i = 0; i < imax; ++i) {
      const double2 p = tab[off + i * u.step];
      const double a = p.x * u.scale, d = p.y * u.scale - a;
      const double wt = a + eta * d;
      acc = (float)((double)acc + wt * (double)xs[n - i]);
    }
    frac = u.scale - frac;
    idx = frac * RS_TABLE;
    off = (int)idx;
    eta = idx - off;
    const int64_t kmax = min(u.in_len - n - 1, (int64_t)((RS_NWIN - off) / u.step));
    for (int64_t k = 0; k < kmax; ++k) {
      const double2 p = tab[off + k * u.step];
      const double a = p.x * u.scale, d = p.y * u.scale - a;
      const double wt = a + eta * d;
      acc = (float)((double)acc + wt * (double)xs[n + 1 + k]);
    }
  }
  y[u.out_off + t] = acc;
}

// the modified Bessel function I0 by its power series, sum ((x/2)^k / k!)^2 (converges fast for x <= 15)
double bessel_i0(double x) {
  const double q = 0.25 * x * x;
  double s = 1.0, term = 1.0;
  for (int k = 1; k < 200; ++k) {
    term *= q / ((double)k * k);
    s += term;
    if (term < s * 1e-17) break;
  }
  return s;
}

}  // namespace

namespace nasr_impl {

// resampy.filters.sinc_window(64, 9, kaiser(beta), rolloff): rolloff * sinc(rolloff * linspace(0, 64, 32769)) times
// the right half of scipy.signal.windows.kaiser(65537, beta)
void resample_filter(double* table) {
  const double pi = 3.14159265358979323846;
  const int half = RS_NWIN - 1;
  const double i0b = bessel_i0(RS_BETA);
  for (int k = 0; k < RS_NWIN; ++k) {
    const double xs = RS_ROLLOFF * ((double)k * ((double)RS_ZEROS / half));
    const double sinc = xs == 0.0 ? 1.0 : std::sin(pi * xs) / (pi * xs);
    const double r = (double)k / half;
    const double win = bessel_i0(RS_BETA * std::sqrt(1.0 - r * r)) / i0b;
    table[k] = RS_ROLLOFF * sinc * win;
  }
}

int64_t resample_length(int32_t in_rate, int32_t out_rate, int64_t n, int64_t* filtered) {
  if (in_rate < 1 || out_rate < 1 || n < 1) return NASR_ERR_ARG;
  if (in_rate == out_rate) {
    if (filtered) *filtered = n;
    return n;
  }
  const double ratio = (double)out_rate / in_rate;
  const double len = (double)n * ratio;
  const int64_t nf = (int64_t)len;
  if (nf < 1) return NASR_ERR_ARG;
  if (filtered) *filtered = nf;
  return (int64_t)std::ceil(len);
}

bool resample_plan(const int64_t* offsets, const int32_t* rates, int n, int32_t out_rate, ResamplePlan* p,
                   std::string* why) {
  p->utt.assign(n, RsUtt{});
  p->waves.clear();
  p->total = 0;
  for (int i = 0; i < n; ++i) {
    const std::string name = "utterance " + std::to_string(i);
    const int64_t len = offsets[i + 1] - offsets[i];
    if (len < 1) return *why = name + " has no samples", false;
    if (rates[i] < 1) return *why = name + ": sample rate " + std::to_string(rates[i]) + " Hz must be > 0", false;
    RsUtt& u = p->utt[i];
    u.in_off = offsets[i] - offsets[0];
    u.in_len = len;
    u.out_off = p->total;
    u.n_samples = resample_length(rates[i], out_rate, len, &u.n_out);
    if (u.n_samples < 1)
      return *why = name + ": " + std::to_string(len) + " samples at " + std::to_string(rates[i]) +
                    " Hz give no sample at " + std::to_string(out_rate) + " Hz (resampy raises)", false;
    const double ratio = (double)out_rate / rates[i];
    u.inc = 1.0 / ratio;
    u.scale = std::min(1.0, ratio);
    u.step = rates[i] == out_rate ? 0 : (int32_t)(u.scale * RS_TABLE);
    double tr = 0.0;
    for (int64_t t = 0; t < u.n_samples; ++t) {
      if (t % RS_WAVE == 0) p->waves.push_back(RsWave{t, tr, i, 0});
      if (u.step && t < u.n_out && (int64_t)tr >= len)    // resampy would read past the input; never seen in practice
        return *why = name + ": the time register leaves the input at output " + std::to_string(t), false;
      if (u.step) tr += u.inc;
    }
    p->total += u.n_samples;
  }
  return true;
}

std::vector<double2> resample_table_pairs() {
  std::vector<double> t(RS_NWIN);
  resample_filter(t.data());
  std::vector<double2> pairs(RS_NWIN);
  for (int k = 0; k < RS_NWIN; ++k) pairs[k] = make_double2(t[k], t[k + 1 < RS_NWIN ? k + 1 : k]);
  return pairs;
}

void launch_resample(const float* x, const RsUtt* utt, const RsWave* waves, int64_t nwaves, const double2* tab2,
                     float* y, hipStream_t st) {
  const int64_t per = RS_THREADS / 64;
  const int64_t nblk = (nwaves + per - 1) / per;
  resample_kernel<<<dim3((unsigned)nblk), dim3(RS_THREADS), 0, st>>>(x, utt, waves, nwaves, tab2, y);
}

}  // namespace nasr_impl

extern "C" {

int nasr_resample_filter(double* table, int64_t len) {
  if (!table || len != RS_NWIN) return NASR_ERR_ARG;
  resample_filter(table);
  return NASR_OK;
}

int64_t nasr_resample_length(int32_t in_rate, int32_t out_rate, int64_t n, int64_t* filtered) {
  return resample_length(in_rate, out_rate, n, filtered);
}

}  // extern "C"
