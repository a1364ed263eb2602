// nasr_fz.h — what a stream session that takes samples (nasr_stream.hip: nasr_stream_attach_audio / _audio_rows /
// _feed_audio) needs of the featurizer handle (nasr_fz.hip; internal, C++).
#pragma once
#include "nasr_ctx.h"
#include "mfcc.h"

namespace nasr_impl {

// What one feed does to every slot, worked out on the host from the sample counts alone; nothing is launched or changed.
struct FzFeedPlan {
  std::vector<FzFeedSlot> slot;
  int64_t seg_total = 0, in_total = 0, f_total = 0, y_total = 0;
  int Tc = 0;
};
// fzh must be a causal featurizer on device `device` whose rows are F wide: NASR_ERR_STATE / NASR_ERR_ARG as the header says
int fz_stream_attach(nasr_ctx* eh, nasr_ctx* fzh, int S, std::unique_ptr<FzStream, FzStreamDelete>* out);
int fz_stream_plan(nasr_ctx* eh, const FzStream& a, const std::string& fn, const int64_t* nnew, const uint8_t* last, FzFeedPlan* p);
// the feed's kernels on stream st; dfeats [S][Tc][F] (NULL with Tc = 0: nothing is emitted) gets the stacked rows, zeros
// behind each slot's
int fz_stream_run(nasr_ctx* eh, FzStream& a, const FzFeedPlan& p, const float* audio, float* dfeats, hipStream_t st);
void fz_stream_advance(FzStream& a, const FzFeedPlan& p, const uint8_t* last);   // the host's counts, once the kernels are queued
void fz_stream_reset(FzStream& a, int slot);                                     // slot < 0: every slot

}  // namespace nasr_impl
