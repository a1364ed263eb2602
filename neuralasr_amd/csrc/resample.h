// resample.h — librosa.load's resampling (reference utils.py:25: librosa.load(wavfile, mono=True, sr=sr)), as librosa
// 0.6-0.9 does it with res_type='kaiser_best': resampy 0.2's band-limited sinc interpolation, then fix_length.
// Host side: the filter table, the lengths, and a plan (per-utterance parameters and the sequential time register at
// the start of every 64 outputs); device side: resample_kernel (resample.hip), one lane per output sample.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>

namespace nasr_impl {

constexpr int RS_ZEROS = 64;                         // kaiser_best: zero crossings of the sinc
constexpr int RS_TABLE = 512;                        // table entries per zero crossing (precision 9)
constexpr int RS_NWIN = RS_ZEROS * RS_TABLE + 1;     // 32769 entries of the right half of the window
constexpr int RS_WAVE = 64;                          // outputs per register checkpoint (one wave)

// resampy's kaiser_best half window in float64 [RS_NWIN]
void resample_filter(double* table);
// librosa's length ceil(n * ratio), and resampy's int(n * ratio) in *filtered; < 0 when resampy raises (no output)
int64_t resample_length(int32_t in_rate, int32_t out_rate, int64_t n, int64_t* filtered);

// One utterance of a launch.  step == 0: the native rate is the target one, the samples are copied (librosa skips
// the resampler).  Otherwise outputs [0, n_out) are filtered and [n_out, n_samples) are fix_length's zeros.
struct RsUtt {
  int64_t in_off, in_len;          // native samples in the input buffer
  int64_t out_off, n_out, n_samples;
  double inc, scale;               // 1 / ratio; min(1, ratio), also the table's factor when ratio < 1
  int32_t step;                    // int(scale * RS_TABLE)
  int32_t pad;
};
// The time register at output t0 of one utterance: tr0 is the value resampy's `tr += inc` loop holds there.
struct RsWave {
  int64_t t0;
  double tr0;
  int32_t u, pad;
};

struct ResamplePlan {
  std::vector<RsUtt> utt;
  std::vector<RsWave> waves;
  int64_t total = 0;               // sum of n_samples: the output buffer's length
};

// The plan of n utterances (audio [offsets[i], offsets[i+1]) at rates[i]) resampled to out_rate; false (and why,
// naming the utterance) on an empty utterance, a rate <= 0 or an utterance too short for one output.
bool resample_plan(const int64_t* offsets, const int32_t* rates, int n, int32_t out_rate, ResamplePlan* p,
                   std::string* why);

// tab2 [RS_NWIN]: (table[k], table[k+1]) pairs, the last one (table[k], table[k]); y [plan total]
void launch_resample(const float* x, const RsUtt* utt, const RsWave* waves, int64_t nwaves, const double2* tab2,
                     float* y, hipStream_t st);
// the pairs of the filter table, as launch_resample reads them
std::vector<double2> resample_table_pairs();

}  // namespace nasr_impl
