// wave_aug.h — the waveform augmentation of a batch given as audio (the reference has none, the rules are
// at nasr_wave_aug in include/nasr.h): reverberation with a room impulse response, then noise at a drawn SNR, on the
// samples at the featurizer's rate.  Host side: the per-utterance parameters and the table of tiles; device side: the
// three kernels of wave_aug.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>

namespace nasr_impl {

constexpr int WV_MAX_TAPS = 8192;                    // NASR_AUG_MAX_RIR_TAPS
constexpr int WV_THREADS = 128;                      // threads of a FIR / mix workgroup
constexpr int WV_PER_THREAD = 8;                     // consecutive outputs a thread owns
constexpr int WV_TILE = WV_THREADS * WV_PER_THREAD;  // outputs per workgroup: 1024, so that a block stays short

// One utterance (the kernels read an array of these as it is).  K == 0: no RIR, the samples are copied.  noise < 0: no
// noise, the mix leaves the samples alone.
struct WvUtt {
  int64_t off, n;                  // its samples in the buffer the kernels read and in the one they write
  int64_t h_off;                   // first tap in the RIR bank
  int64_t c_off, c_len, c_pos;     // the clip in the noise bank, its length L, the offset o
  double scale;                    // 10^(-snr_db / 20)
  int64_t tile0;                   // its first tile in the table (wave_tiles)
  int32_t K, noise;
};
// One tile: outputs [t0, t0 + WV_TILE) of utterance u
struct WvTile {
  int64_t t0;
  int32_t u, pad;
};

struct WavePlan {
  std::vector<WvUtt> utt;
  std::vector<WvTile> tiles;
  size_t bytes() const { return utt.size() * sizeof(WvUtt) + tiles.size() * sizeof(WvTile); }
};

// the tiles of utt, utterance after utterance, and every utterance's tile0
void wave_tiles(WavePlan* p);

// x -> y out of place (wave_fir_kernel: the RIR, or the copy; part [ntiles][2] gets the tiles' shares of the two powers),
// gain [n] (wave_gain_kernel), y in place (wave_mix_kernel).  taps / clips: the banks (nullable when no utterance uses them).
void launch_wave_aug(const float* x, float* y, const WvUtt* utt, int n, const WvTile* tiles, int64_t ntiles,
                     const float* taps, const float* clips, double* part, float* gain, hipStream_t st);

}  // namespace nasr_impl
