// mfcc.h — the feature front end's kernels (mfcc.hip; internal, C++): what a host caller needs to run them.  The host-side
// arithmetic that is a pure function of nasr_mfcc_cfg (the checks, psf's frame count, the filterbank, the tables), the
// descriptor a stream feed hands to the kernels, and one launcher per kernel.  The handle that owns the buffers and
// decides what is launched when is nasr_fz.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/nasr.h"

namespace nasr_impl {

struct FzDims {
  int frame_len, frame_step, numcep, nfilt, nc;
  int append_energy;
  float preemph;
  int kind, width;                      // cfg.kind; D = numcep (1 + deltas), the row stride of the cep buffer
};

// tw [256] = exp(-2 pi i t / 256), tw2 [257] = exp(-2 pi i k / 512); fb_lo/fb_n [nfilt]: a filter's first bin and bin
// count, fb_off [nfilt]: where its weights start in fb_w; dct [nfilt][numcep]: ortho DCT-II x lifter, c fastest.
struct FzTables {
  const double2 *tw, *tw2;
  const int *fb_lo, *fb_n, *fb_off;
  const double *fb_w, *dct;
};
// the same tables as they are built on the host, in double (once per handle)
struct FzHostTables {
  std::vector<double2> tw, tw2;
  std::vector<int> fb_lo, fb_n, fb_off;
  std::vector<double> fb_w, dct;
};
FzHostTables fz_host_tables(const nasr_mfcc_cfg* c);

bool cfg_ok(const nasr_mfcc_cfg* c, std::string* why);
int64_t round_half_up(double x);                                 // psf round_half_up, x >= 0
int64_t frames_of(int64_t flen, int64_t fstep, int64_t n);       // psf's frame count of n >= 1 samples
std::vector<double> filter_bins(const nasr_mfcc_cfg* c);         // [nfilt + 2]
std::vector<double> filter_weights(const nasr_mfcc_cfg* c, const std::vector<double>& bin);   // dense [nfilt][nfft/2+1]

// What one feed of a stream session that takes samples does to a slot, worked out on the host from the sample counts alone
// (nasr_fz.hip: fz_stream_plan).
struct FzFeedSlot {
  // (int64 throughout: the kernels read an array of these as it is)
  int64_t seg_off, ntail, in_off, nnew;   // the slot's segment of the work buffer: ntail carried samples, then nnew new ones
  int64_t keep_off, nkeep;                // the part of the segment that is the next feed's tail
  int64_t lead;                           // samples of the segment in front of the first new frame (0 or 1)
  int64_t f_off, nfb, want;               // first new frame in the work buffers; frames before and after the feed
  int64_t nnorm, upto, y_off;             // frames normalised before and after; first of them in the work buffer
  int64_t T;                              // the utterance's frames when this feed completes it, else -1
  int64_t rows0, nrows;                   // rows emitted before, and by this feed
  int64_t n_after;                        // samples received after the feed
};

// mfcc_spectral_kernel: every frame of the batch, one wave each.  uoff [n+1] (int64 sample offsets), foff [n+1] (int64
// frame offsets), fmap [nframes] (frame -> utterance), ulead (NULL: zeros) [n]: the samples of an utterance in front of
// its first frame of this launch.  cep [nframes][d.width] gets the static columns.
void launch_mfcc_spectral(const float* audio, const int64_t* uoff, const int64_t* foff, const int* fmap, const int64_t* ulead,
                          int64_t nframes, const FzTables& t, const FzDims& d, double* cep, hipStream_t st);
// mfcc_delta_kernel: one level of psf's delta(feat, 2), columns [src, src + numcep) of every frame into [dst, dst + numcep)
void launch_mfcc_delta(double* cep, const int64_t* foff, const int* fmap, int64_t nframes, int numcep, int width, int src, int dst,
                       hipStream_t st);
// mfcc_norm_kernel: one workgroup per utterance, frames [n][.][D] at cep.  rule: cfg.norm (0: the whole-utterance mean and
// std; 1: the causal rule with M = norm_min_frames, pfx and ms [F][2] its scratch).  slot false: the stacked rows
// [F][(2 nc + 1) D] into out and every utterance's (mean, std) into mstd (nullable).  slot true: the centre frames
// [n][Tb][D] into out, zeros past each utterance's end, and its out-of-utterance value into pad [n].
void launch_mfcc_norm(const double* cep, const int64_t* foff, int n, int D, int nc, int rule, int M, double* pfx, double* ms,
                      bool slot, int Tb, float* out, float* pad, double* mstd, hipStream_t st);
// the four kernels of a stream feed, S slots described by desc; longest >= 1: the most samples (tail + new) of a slot
void launch_mfcc_stream_assemble(const FzFeedSlot* desc, int S, int64_t longest, const float* tail, int tail_cap, const float* in,
                                 float* seg, hipStream_t st);
void launch_mfcc_stream_norm(const double* cep, const FzFeedSlot* desc, int S, int D, int M, double* sums, double* pend,
                             double* pfx, float* ynew, hipStream_t st);
void launch_mfcc_stream_stack(const FzFeedSlot* desc, int S, int Tc, int D, int nc, int R, const float* ynew, const float* yring,
                              float* out, hipStream_t st);
void launch_mfcc_stream_carry(const FzFeedSlot* desc, int S, int D, int nc, int R, const float* ynew, float* yring,
                              const float* seg, float* tail, int tail_cap, hipStream_t st);

}  // namespace nasr_impl
