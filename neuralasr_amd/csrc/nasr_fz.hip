// nasr_fz.hip — the featurizer handle (nasr_create_featurizer; reference utils.py:24-31, convert_to_mfcc): the front end's
// tables and scratch buffers, what a call works out on the host before anything is launched, and the order in which the
// kernels of mfcc.hip, resample.hip and wave_aug.hip run.  Three kinds of call end here:
//   calls that return to the host (nasr_featurize, nasr_featurize_rates, nasr_resample, nasr_augment_audio): on the
//       featurizer's own stream, waited for;
//   batch-slot calls (nasr_upload_batch_audio*, nasr_stage_batch_audio*): the front end as the device producer of a MODEL
//       handle's batch slot, on that handle's stream, returning with the kernels in flight;
//   a stream session that takes samples (nasr_stream_attach_audio / _feed_audio; FzStream): per slot the sample tail, the
//       running sums, the frames that wait and the ring of recent ones, fed on the model's stream as well.
// Every call is fz_plan (the resampling plan, the offsets, the augmentation plan and what is sent to the device: Staging),
// then fz_front (the copies, the resampler, the augmentation, mfcc_spectral_kernel, the deltas), then the normaliser into
// the layout that the call wants, then one of two tails.  nasr_featurize_rates first resamples utterances at other rates
// to the config rate into a device buffer, which the same kernels then read; a call with waveform augmentation
//  runs wave_aug.hip's three kernels behind the resampler, and the spectral kernel reads their output.
#include "nasr_fz.h"
#include "resample.h"
#include "wave_aug.h"

using namespace nasr;
using namespace nasr_impl;

namespace nasr_impl {

struct FzState {
  nasr_mfcc_cfg cfg;
  FzDims d;
  int W = 1;
  DevPtr<double2> tw, tw2;
  DevPtr<int> fb_lo, fb_n, fb_off;
  DevPtr<double> fb_w, dct;
  FzTables tables() const { return FzTables{tw.get(), tw2.get(), fb_lo.get(), fb_n.get(), fb_off.get(), fb_w.get(), dct.get()}; }
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

void FzStateDelete::operator()(FzState* f) const { delete f; }

}  // namespace nasr_impl

namespace {

// The featurizer behind the handle of ABI call fn; NULL with *rc set when there is none (a null handle: NASR_ERR_ARG)
FzState* fz_of(nasr_handle h, const std::string& fn, int* rc) {
  if (!h) return *rc = NASR_ERR_ARG, nullptr;
  if (!h->fz) return *rc = h->fail(NASR_ERR_STATE, fn + ": not a featurizer handle"), nullptr;
  return h->fz.get();
}

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

// The tail of a call that leaves its kernels in flight on a model handle's stream st (rc: what queuing them came to).  Also
// when something failed part-way: whatever was queued on st still reads the scratch buffers.
int scratch_release(FzState& z, hipStream_t st, int rc) {
  (void)hipEventRecord(z.ev[2], st);
  if (hipEventRecord(z.ev_busy, st) == hipSuccess) z.busy_valid = true;
  z.times_pending = rc == NASR_OK;       // nasr_featurize_times: this call's copies and front-end kernels
  return rc;
}

// The tail of a call that returns to the host: `bytes` from dsrc to `out` (and bytes2 from dsrc2 to out2 when out2 is
// given), the wait for the stream, and the device-timed phases between the four events.
int return_to_host(nasr_ctx* h, FzState& z, void* out, const void* dsrc, size_t bytes, void* out2 = nullptr,
                   const void* dsrc2 = nullptr, size_t bytes2 = 0) {
  HIPCHK(h, hipEventRecord(z.ev[2], h->st));
  HIPCHK(h, hipMemcpyAsync(out, dsrc, bytes, hipMemcpyDeviceToHost, h->st));
  if (out2) HIPCHK(h, hipMemcpyAsync(out2, dsrc2, bytes2, hipMemcpyDeviceToHost, h->st));
  HIPCHK(h, hipEventRecord(z.ev[3], h->st));
  if (int rc = sync_checked(h)) return rc;
  for (int i = 0; i < 3; ++i)
    if (hipEventElapsedTime(&z.times[i], z.ev[i], z.ev[i + 1]) != hipSuccess) z.times[i] = 0.f;
  z.times_pending = false;
  return NASR_OK;
}

// ------------------------------------------------------------------------------------------------------- staging
// What a call sends to the device: its segments in the order they are copied, each with its host source, its byte count
// and the scratch buffer it goes to.  A segment without bytes is not sent.
struct Staging {
  struct Seg {
    const void* src = nullptr;
    size_t bytes = 0;
    DevBuf* dst = nullptr;
  };
  Seg seg[4];
  int n = 0;
  void add(const void* src, size_t bytes, DevBuf& dst) { seg[n++] = Seg{src, bytes, &dst}; }
  // In pinned memory the segments stand one behind the other, the first (the samples) rounded up to 8 bytes.
  static size_t stride(int i, size_t bytes) { return i == 0 ? (bytes + 7) / 8 * 8 : bytes; }
  size_t pinned_bytes() const {
    size_t b = 0;
    for (int i = 0; i < n; ++i) b += stride(i, seg[i].bytes);
    return b;
  }
  // the segments into `pinned` (pinned_bytes() of it), which they are then sent from: plain DMAs that return at once
  void pack(void* pinned) {
    char* q = static_cast<char*>(pinned);
    for (int i = 0; i < n; ++i) {
      if (seg[i].bytes) memcpy(q, seg[i].src, seg[i].bytes);
      seg[i].src = q;
      q += stride(i, seg[i].bytes);
    }
  }
  int copy(nasr_ctx* eh, hipStream_t st) const {
    for (int i = 0; i < n; ++i)
      if (seg[i].bytes) HIPCHK(eh, hipMemcpyAsync(seg[i].dst->p, seg[i].src, seg[i].bytes, hipMemcpyHostToDevice, st));
    return NASR_OK;
  }
};

// A segment's host image: the parts one behind the other.  A part without a source is room that the caller fills.
struct Part {
  const void* p;
  size_t bytes;
};
char* image(std::vector<char>& img, std::initializer_list<Part> parts) {
  size_t total = 0;
  for (const Part& s : parts) total += s.bytes;
  img.resize(total);
  char* q = img.data();
  for (const Part& s : parts) {
    if (s.p) memcpy(q, s.p, s.bytes);
    q += s.bytes;
  }
  return img.data();
}

// ---------------------------------------------------------------------------------------------------------- plan
// What a front-end call works out on the host before anything is launched.
struct FzPlan {
  ResamplePlan rp;
  bool rs = false;                     // some utterance is resampled: the kernels read the resampled buffer
  int n = 0;
  std::vector<int64_t> uoff, foff;     // [n+1] sample offsets (in the buffer the kernels read) and frame offsets
  int64_t S_in = 0;                    // native samples
  bool wave = false;                   // waveform augmentation: wp is filled, the kernels read its output
  WavePlan wp;
  bool feats = true;                   // false: the call wants the samples at the featurizer's rate, and no features
  // the samples; with feats the meta block (uoff, foff, then fmap [F]: int32 frame -> utterance); the resampling plan
  // (RsUtt [n], then RsWave [waves]) and the augmentation plan (WvUtt [n], then WvTile [tiles]) when there is one
  Staging stage;
  const int64_t* d_foff(const FzState& z) const { return z.meta.as<int64_t>() + (n + 1); }
  const int* d_fmap(const FzState& z) const { return reinterpret_cast<const int*>(z.meta.as<int64_t>() + 2 * (n + 1)); }
};

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

// The plan of ABI call fn: the resampling plan (rates nullable: every utterance is at the config rate), every utterance's
// sample and frame offsets, the checks and parameters of `wave` (nullable), and the staging, whose host images are left in
// z.  audio: the first utterance's first sample.  Errors go to handle eh (the featurizer itself, or the model handle of a
// batch-slot call).
int fz_plan(nasr_ctx* eh, FzState& z, const std::string& fn, const float* audio, const int64_t* offsets, const int32_t* rates, int n,
            const nasr_wave_aug* wave, bool feats, FzPlan* p) {
  p->rs = false;
  p->feats = feats;
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
  if (int rc = fz_wave_plan(eh, z, fn, wave, p)) return rc;

  Staging& s = p->stage;
  s.add(audio, (size_t)p->S_in * 4, z.audio);
  if (feats) {
    const size_t ob = (size_t)(n + 1) * 8, fb = (size_t)p->foff[n] * 4;
    char* m = image(z.hmeta, {{p->uoff.data(), ob}, {p->foff.data(), ob}, {nullptr, fb}});
    int* fmap = reinterpret_cast<int*>(m + 2 * ob);
    for (int i = 0; i < n; ++i)
      for (int64_t f = p->foff[i]; f < p->foff[i + 1]; ++f) fmap[f] = i;
    s.add(m, 2 * ob + fb, z.meta);
  }
  if (p->rs) {
    const size_t ub = p->rp.utt.size() * sizeof(RsUtt), wb = p->rp.waves.size() * sizeof(RsWave);
    s.add(image(z.hrmeta, {{p->rp.utt.data(), ub}, {p->rp.waves.data(), wb}}), ub + wb, z.rmeta);
  }
  if (p->wave) {
    const size_t ub = p->wp.utt.size() * sizeof(WvUtt);
    s.add(image(z.hwmeta, {{p->wp.utt.data(), ub}, {p->wp.tiles.data(), p->wp.bytes() - ub}}), p->wp.bytes(), z.wmeta);
  }
  return NASR_OK;
}

// The copies, the resampler, the augmentation, mfcc_spectral_kernel and the delta launches of plan p on stream st: z.cep
// holds the frames [F][D] afterwards, z.meta the offsets.  pinned (nullable): p.stage.pinned_bytes() of pinned memory the
// host-to-device copies go through.  Without p.feats it returns behind the last kernel that writes the samples at the
// featurizer's rate, augmented when the plan says so, with *samples_out where they are.
int fz_front(nasr_ctx* eh, FzState& z, const std::string& fn, const FzPlan& p, void* pinned, hipStream_t st,
             const float** samples_out = nullptr) {
  const int n = p.n;
  const int64_t F = p.foff[n];
  if (int rc = scratch_acquire(eh, z, st)) return rc;
  if (p.rs) {                            // the filter table (once per handle) and the device buffers of a resampling launch
    if (!z.rs_tab) {
      const std::vector<double2> pairs = resample_table_pairs();
      HIPCHK(eh, hipMalloc(z.rs_tab.out(), pairs.size() * sizeof(double2)));
      HIPCHK(eh, hipMemcpy(z.rs_tab.get(), pairs.data(), pairs.size() * sizeof(double2), hipMemcpyHostToDevice));
    }
    if (!scratch_ensure(z, z.audio, (size_t)p.S_in * 4) || !scratch_ensure(z, z.raud, (size_t)p.rp.total * 4) ||
        !scratch_ensure(z, z.rmeta, z.hrmeta.size()))
      return eh->fail(NASR_ERR_HIP, "resampling: device buffers for " + std::to_string(p.S_in) + " + " +
                                        std::to_string(p.rp.total) + " samples could not be allocated");
  }
  if (!scratch_ensure(z, z.audio, (size_t)p.S_in * 4) ||
      (p.feats && (!scratch_ensure(z, z.meta, z.hmeta.size()) || !scratch_ensure(z, z.cep, (size_t)F * z.d.width * 8) ||
                   !scratch_ensure(z, z.mstd, (size_t)n * 16))) ||
      (p.feats && z.cfg.norm == 1 && (!scratch_ensure(z, z.pfx, (size_t)F * 16) || !scratch_ensure(z, z.fms, (size_t)F * 16))))
    return eh->fail(NASR_ERR_HIP, fn + ": device buffers for " + std::to_string(p.uoff[n]) + " samples could not be allocated");
  if (p.wave) {
    if (!scratch_ensure(z, z.wav, (size_t)p.uoff[n] * 4) || !scratch_ensure(z, z.wmeta, p.wp.bytes()) ||
        !scratch_ensure(z, z.wpart, p.wp.tiles.size() * 16) || !scratch_ensure(z, z.gain, (size_t)n * 4))
      return eh->fail(NASR_ERR_HIP, fn + ": device buffers for " + std::to_string(p.uoff[n]) + " augmented samples could not be allocated");
  }
  Staging stage = p.stage;
  if (pinned) stage.pack(pinned);
  HIPCHK(eh, hipEventRecord(z.ev[0], st));
  if (int rc = stage.copy(eh, st)) return rc;
  HIPCHK(eh, hipEventRecord(z.ev[1], st));
  if (p.rs) {
    launch_resample(z.audio.as<float>(), z.rmeta.as<RsUtt>(), reinterpret_cast<const RsWave*>(z.rmeta.as<RsUtt>() + n),
                    (int64_t)p.rp.waves.size(), z.rs_tab, z.raud.as<float>(), st);
    HIPCHK(eh, hipGetLastError());
  }
  const float* samples = p.rs ? z.raud.as<float>() : z.audio.as<float>();
  if (p.wave) {
    launch_wave_aug(samples, z.wav.as<float>(), z.wmeta.as<WvUtt>(), n, reinterpret_cast<const WvTile*>(z.wmeta.as<WvUtt>() + n),
                    (int64_t)p.wp.tiles.size(), z.rir_bank.as<float>(), z.noise_bank.as<float>(), z.wpart.as<double>(),
                    z.gain.as<float>(), st);
    HIPCHK(eh, hipGetLastError());
    samples = z.wav.as<float>();
  }
  if (!p.feats) {
    *samples_out = samples;
    return NASR_OK;
  }
  launch_mfcc_spectral(samples, z.meta.as<int64_t>(), p.d_foff(z), p.d_fmap(z), nullptr, F, z.tables(), z.d, z.cep.as<double>(), st);
  HIPCHK(eh, hipGetLastError());
  for (int lv = 1; lv <= z.cfg.deltas; ++lv) {
    launch_mfcc_delta(z.cep.as<double>(), p.d_foff(z), p.d_fmap(z), F, z.d.numcep, z.d.width, (lv - 1) * z.d.numcep,
                      lv * z.d.numcep, st);
    HIPCHK(eh, hipGetLastError());
  }
  return NASR_OK;
}

// The normaliser of the featurizer's rule behind fz_front, on stream st: the stacked rows into z.out and the statistics
// into z.mstd, or (slot) the centre frames of a batch slot [n][Tb][D] into out and the pad values into pad.
void fz_norm(FzState& z, const FzPlan& p, bool slot, int Tb, float* out, float* pad, hipStream_t st) {
  launch_mfcc_norm(z.cep.as<double>(), p.d_foff(z), p.n, z.d.width, z.d.nc, z.cfg.norm, z.cfg.norm_min_frames, z.pfx.as<double>(),
                   z.fms.as<double>(), slot, Tb, out, pad, slot ? nullptr : z.mstd.as<double>(), st);
}

// The device producer of a batch slot's centre frames (nasr_batch.hip slot_fill): the front end of plan p on the slot's
// stream, then the normaliser straight into the slot.  The featurizer's scratch buffers are busy until ev_busy.
int fz_produce_slot(nasr_ctx* eh, nasr_ctx* fzh, const FzPlan& p, int Tb, float* dcentre, float* dpad, void* pinned,
                    hipStream_t st) {
  FzState& z = *fzh->fz;
  const std::string fn = "audio batch";
  int rc = fz_front(eh, z, fn, p, pinned, st);
  if (!rc) {
    fz_norm(z, p, true, Tb, dcentre, dpad, st);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) rc = eh->fail(NASR_ERR_HIP, fn + ": " + hipGetErrorString(e));
  }
  return scratch_release(z, st, rc);
}

// The features of n utterances.  rates == nullptr (nasr_featurize): every utterance is at the config rate.  Otherwise
// an utterance at another rate is resampled to it first, into z.raud, which the MFCC kernels then read.
int featurize(nasr_handle h, const std::string& fn, const float* audio, const int64_t* offsets, const int32_t* rates,
              int n, float* out, int64_t out_rows, double* mean_std) {
  int rc = NASR_OK;
  FzState* zp = fz_of(h, fn, &rc);
  if (!zp) return rc;
  FzState& z = *zp;
  if (!audio || !offsets || !out || n < 1) return h->fail(NASR_ERR_ARG, fn + ": null buffer or n < 1");
  FzPlan p;
  if (int rc = fz_plan(h, z, fn, audio + offsets[0], offsets, rates, n, nullptr, true, &p)) return rc;
  const int64_t F = p.foff[n];
  if (out_rows != F)
    return h->fail(NASR_ERR_ARG, fn + ": out_rows is " + std::to_string(out_rows) + ", the utterances have " +
                                     std::to_string(F) + " frames");
  const size_t rowlen = (size_t)z.W * z.d.width;
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = scratch_acquire(h, z, h->st)) return rc;
  if (!z.out.ensure((size_t)F * rowlen * 4, nullptr))
    return h->fail(NASR_ERR_HIP, fn + ": device buffers for " + std::to_string(p.uoff[n]) + " samples could not be allocated");
  if (int rc = fz_front(h, z, fn, p, nullptr, h->st)) return rc;
  fz_norm(z, p, false, 0, z.out.as<float>(), nullptr, h->st);
  HIPCHK(h, hipGetLastError());
  return return_to_host(h, z, out, z.out.p, (size_t)F * rowlen * 4, mean_std, z.mstd.p, (size_t)n * 16);
}

// nasr_resample and nasr_augment_audio (fn: the one that was called): the samples at the featurizer's rate, resampled and
// (wave, nullable) augmented on the device, back to the host.  need_rates: nasr_resample, whose rates are no option and
// whose out_len message has its own words.
int samples_to_host(nasr_handle h, const std::string& fn, const float* audio, const int64_t* offsets, const int32_t* rates,
                    bool need_rates, int n, const nasr_wave_aug* wave, float* out, int64_t out_len) {
  int rc = NASR_OK;
  FzState* zp = fz_of(h, fn, &rc);
  if (!zp) return rc;
  FzState& z = *zp;
  if (!audio || !offsets || (need_rates && !rates) || !out || n < 1) return h->fail(NASR_ERR_ARG, fn + ": null buffer or n < 1");
  FzPlan p;
  if (int rc = fz_plan(h, z, fn, audio + offsets[0], offsets, rates, n, wave, false, &p)) return rc;
  if (out_len != p.uoff[n])
    return h->fail(NASR_ERR_ARG, fn + ": out_len is " + std::to_string(out_len) + ", the utterances " +
                                     (need_rates ? "resample to " + std::to_string(p.uoff[n]) + " samples"
                                                 : "have " + std::to_string(p.uoff[n]) + " samples at the featurizer's rate"));
  HIPCHK(h, hipSetDevice(h->device));
  const float* samples = nullptr;
  if (int rc = fz_front(h, z, fn, p, nullptr, h->st, &samples)) return rc;
  return return_to_host(h, z, out, samples, (size_t)out_len * 4);
}

// A bank of the featurizer (noise clips, RIRs): the checks, then the upload; `what` names an entry in the messages.
int set_bank(nasr_ctx* h, const std::string& fn, const char* what, const float* data, const int64_t* offsets, int n,
             int64_t max_len, DevBuf FzState::*bank, std::vector<int64_t> FzState::*off) {
  int rc = NASR_OK;
  FzState* zp = fz_of(h, fn, &rc);
  if (!zp) return rc;
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

// The six nasr_*_batch_audio* calls (utils.py:24-31 feeding dataset.py:33-40), fn the one that was called: the checks, the
// host-side plan (seq_len, T), and the front end as the producer of the slot's centre frames.  staged: into *ticket.
int audio_batch(const std::string& fn, nasr_ctx* h, nasr_ctx* fzh, const float* audio, const int64_t* offsets,
                const int32_t* rates, const int32_t* labels, const int32_t* label_len, int B, int Lmax, int32_t* seq_len_out,
                int* T_out, const nasr_batch_aug* aug, const nasr_wave_aug* wave, bool staged, int* ticket) {
  if (!h) return NASR_ERR_ARG;
  if (h->family == Family::Featurizer) return h->fail(NASR_ERR_STATE, fn + ": a featurizer handle has no model");   // MODEL_CALL
  if (staged) {
    if (!ticket) return h->fail(NASR_ERR_ARG, "null ticket");
    *ticket = -1;
  }
  if (!fzh || !fzh->fz) return h->fail(NASR_ERR_STATE, fn + ": `featurizer` is not a featurizer handle");
  if (fzh->device != h->device)
    return h->fail(NASR_ERR_STATE, fn + ": the model is on device " + std::to_string(h->device) + ", the featurizer on device " +
                                       std::to_string(fzh->device));
  if (!audio || !offsets || !seq_len_out || !T_out) return h->fail(NASR_ERR_ARG, fn + ": null buffer");
  if (B < 1 || B > 64) return validate_batch(h, nullptr, nullptr, nullptr, B, 1, 0);
  FzState& z = *fzh->fz;
  const int ctx = z.d.nc, ncep = z.d.width;   // ncep: the featurizer's frame width, numcep*(1+deltas)
  if (z.W * ncep != h->F)
    return h->fail(NASR_ERR_ARG, fn + ": feature_size " + std::to_string(h->F) + " must equal (2*numcontext+1)*numcep*(1+deltas) = (2*" +
                                     std::to_string(ctx) + "+1)*" + std::to_string(ncep) + " of the featurizer");
  if (aug && aug->static_width != z.d.numcep)
    return h->fail(NASR_ERR_ARG, fn + ": augmentation: static_width " + std::to_string(aug->static_width) +
                                     " is not the featurizer's numcep " + std::to_string(z.d.numcep));
  FzPlan plan;
  if (int rc = fz_plan(h, z, fn, audio + offsets[0], offsets, rates, B, wave, true, &plan)) return rc;
  int64_t Tmax = 0;
  for (int b = 0; b < B; ++b) Tmax = std::max(Tmax, plan.foff[b + 1] - plan.foff[b]);
  if (Tmax > (1 << 24)) return h->fail(NASR_ERR_ARG, fn + ": an utterance of " + std::to_string(Tmax) + " frames");
  const int T = (int)Tmax;
  for (int b = 0; b < B; ++b) seq_len_out[b] = (int32_t)(plan.foff[b + 1] - plan.foff[b]);
  *T_out = T;
  CentreProducer prod;
  prod.stage_bytes = plan.stage.pinned_bytes();
  prod.run = [&](float* dcentre, float* dpad, void* pinned, hipStream_t cs) {
    return fz_produce_slot(h, fzh, plan, T, dcentre, dpad, pinned, cs);
  };
  const BatchSrc src = produced_batch(&prod, ctx, ncep, seq_len_out, labels, label_len, B, T, Lmax, aug);
  return staged ? stage(h, src, ticket) : upload(h, src);
}

}  // namespace

namespace nasr_impl {

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
  char* m = image(z.hmeta, {{p.slot.data(), db}, {nullptr, 2 * ob + (size_t)S * 8 + (size_t)F * 4}});
  int64_t* uoff = reinterpret_cast<int64_t*>(m + db);
  int64_t* foff = uoff + (S + 1);
  int64_t* lead = foff + (S + 1);
  int* fmap = reinterpret_cast<int*>(lead + S);
  int64_t longest = 1;
  for (int b = 0; b < S; ++b) {
    const FzFeedSlot& d = p.slot[(size_t)b];
    uoff[b] = d.seg_off;
    foff[b] = d.f_off;
    lead[b] = d.lead;
    for (int64_t f = 0; f < d.want - d.nfb; ++f) fmap[d.f_off + f] = b;
    longest = std::max(longest, d.ntail + d.nnew);
  }
  uoff[S] = p.seg_total;
  foff[S] = F;
  Staging stage;
  stage.add(audio, (size_t)p.in_total * 4, z.sin);
  stage.add(m, z.hmeta.size(), z.meta);
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
    if (int rc = stage.copy(eh, st)) return rc;
    HIPCHK(eh, hipEventRecord(z.ev[1], st));
    launch_mfcc_stream_assemble(desc, S, longest, a.tail.as<float>(), a.tail_cap, z.sin.as<float>(), z.audio.as<float>(), st);
    HIPCHK(eh, hipGetLastError());
    if (F > 0) {
      launch_mfcc_spectral(z.audio.as<float>(), d_uoff, d_uoff + (S + 1), reinterpret_cast<const int*>(d_uoff + 3 * S + 2),
                           d_uoff + 2 * (S + 1), F, z.tables(), z.d, z.cep.as<double>(), st);
      HIPCHK(eh, hipGetLastError());
    }
    launch_mfcc_stream_norm(z.cep.as<double>(), desc, S, D, z.cfg.norm_min_frames, a.sums.as<double>(), a.pend.as<double>(),
                            z.pfx.as<double>(), z.ynew.as<float>(), st);
    HIPCHK(eh, hipGetLastError());
    if (dfeats) {
      launch_mfcc_stream_stack(desc, S, p.Tc, D, z.d.nc, a.R, z.ynew.as<float>(), a.yring.as<float>(), dfeats, st);
      HIPCHK(eh, hipGetLastError());
    }
    launch_mfcc_stream_carry(desc, S, D, z.d.nc, a.R, z.ynew.as<float>(), a.yring.as<float>(), z.audio.as<float>(),
                             a.tail.as<float>(), a.tail_cap, st);
    HIPCHK(eh, hipGetLastError());
    return NASR_OK;
  };
  return scratch_release(z, st, queue());
}

}  // namespace nasr_impl

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
  const FzHostTables t = fz_host_tables(cfg);
  auto put = [&](auto& dst, const auto& v) {
    using T = typename std::decay_t<decltype(v)>::value_type;
    if (hipMalloc(dst.out(), v.size() * sizeof(T)) != hipSuccess) return false;
    return hipMemcpy(dst.get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
  };
  if (!put(z.tw, t.tw) || !put(z.tw2, t.tw2) || !put(z.fb_lo, t.fb_lo) || !put(z.fb_n, t.fb_n) || !put(z.fb_off, t.fb_off) ||
      !put(z.fb_w, t.fb_w) || !put(z.dct, t.dct))
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
  return samples_to_host(h, __func__, audio, offsets, rates, true, n, nullptr, out, out_len);
}

int nasr_augment_audio(nasr_handle h, const float* audio, const int64_t* offsets, const int32_t* rates, int n,
                       const nasr_wave_aug* wave, float* out, int64_t out_len) {
  return samples_to_host(h, __func__, audio, offsets, rates, false, n, wave, out, out_len);
}

int nasr_featurizer_set_noise(nasr_handle h, const float* samples, const int64_t* offsets, int n_clips) {
  return set_bank(h, __func__, "noise clip", samples, offsets, n_clips, 0, &FzState::noise_bank, &FzState::noise_off);
}

int nasr_featurizer_set_rirs(nasr_handle h, const float* taps, const int64_t* offsets, int n_rirs) {
  return set_bank(h, __func__, "RIR", taps, offsets, n_rirs, WV_MAX_TAPS, &FzState::rir_bank, &FzState::rir_off);
}

int nasr_featurize_times(nasr_handle h, float* h2d_ms, float* kernel_ms, float* d2h_ms) {
  int rc = NASR_OK;
  FzState* zp = fz_of(h, __func__, &rc);
  if (!zp) return rc;
  FzState& z = *zp;
  if (z.times_pending) {                 // a batch-slot call: copies and kernels on the model's stream, nothing comes back
    HIPCHK(h, hipEventSynchronize(z.ev[2]));
    for (int i = 0; i < 2; ++i)
      if (hipEventElapsedTime(&z.times[i], z.ev[i], z.ev[i + 1]) != hipSuccess) z.times[i] = 0.f;
    z.times[2] = 0.f;
    z.times_pending = false;
  }
  if (h2d_ms) *h2d_ms = z.times[0];
  if (kernel_ms) *kernel_ms = z.times[1];
  if (d2h_ms) *d2h_ms = z.times[2];
  return NASR_OK;
}

int nasr_upload_batch_audio(nasr_handle model, nasr_handle featurizer, const float* audio, const int64_t* offsets,
                            const int32_t* rates, const int32_t* labels, const int32_t* label_len, int B, int Lmax,
                            int32_t* seq_len_out, int* T_out) {
  return audio_batch(__func__, model, featurizer, audio, offsets, rates, labels, label_len, B, Lmax, seq_len_out, T_out, nullptr,
                     nullptr, false, nullptr);
}

int nasr_stage_batch_audio(nasr_handle model, nasr_handle featurizer, const float* audio, const int64_t* offsets,
                           const int32_t* rates, const int32_t* labels, const int32_t* label_len, int B, int Lmax,
                           int32_t* seq_len_out, int* T_out, int* ticket) {
  return audio_batch(__func__, model, featurizer, audio, offsets, rates, labels, label_len, B, Lmax, seq_len_out, T_out, nullptr,
                     nullptr, true, ticket);
}

int nasr_upload_batch_audio_aug(nasr_handle model, nasr_handle featurizer, const float* audio, const int64_t* offsets,
                                const int32_t* rates, const int32_t* labels, const int32_t* label_len, int B, int Lmax,
                                int32_t* seq_len_out, int* T_out, const nasr_batch_aug* aug) {
  return audio_batch(__func__, model, featurizer, audio, offsets, rates, labels, label_len, B, Lmax, seq_len_out, T_out, aug,
                     nullptr, false, nullptr);
}

int nasr_stage_batch_audio_aug(nasr_handle model, nasr_handle featurizer, const float* audio, const int64_t* offsets,
                               const int32_t* rates, const int32_t* labels, const int32_t* label_len, int B, int Lmax,
                               int32_t* seq_len_out, int* T_out, const nasr_batch_aug* aug, int* ticket) {
  return audio_batch(__func__, model, featurizer, audio, offsets, rates, labels, label_len, B, Lmax, seq_len_out, T_out, aug,
                     nullptr, true, ticket);
}

int nasr_upload_batch_audio_wave(nasr_handle model, nasr_handle featurizer, const float* audio, const int64_t* offsets,
                                 const int32_t* rates, const int32_t* labels, const int32_t* label_len, int B, int Lmax,
                                 int32_t* seq_len_out, int* T_out, const nasr_batch_aug* aug, const nasr_wave_aug* wave) {
  return audio_batch(__func__, model, featurizer, audio, offsets, rates, labels, label_len, B, Lmax, seq_len_out, T_out, aug,
                     wave, false, nullptr);
}

int nasr_stage_batch_audio_wave(nasr_handle model, nasr_handle featurizer, const float* audio, const int64_t* offsets,
                                const int32_t* rates, const int32_t* labels, const int32_t* label_len, int B, int Lmax,
                                int32_t* seq_len_out, int* T_out, const nasr_batch_aug* aug, const nasr_wave_aug* wave,
                                int* ticket) {
  return audio_batch(__func__, model, featurizer, audio, offsets, rates, labels, label_len, B, Lmax, seq_len_out, T_out, aug,
                     wave, true, ticket);
}

}  // extern "C"
