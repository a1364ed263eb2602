// nasr_stream.hip — streaming sessions on a unidirectional LSTM handle (nasr_stream_*).  The reference
// decodes whole utterances (networks/tfnetwork.py:179-181); a session keeps each stream's recurrent state (c, h) per layer
// on the device between chunks, so that a causal network recognises audio as it arrives.  A feed is an ordinary forward
// pass over the chunk (nasr_pass.hip: forward(h, true)) whose recurrence starts from the saved state and saves it again
// (lstm.hip: the state-carrying step, stream_load_state_kernel, stream_save_state_kernel).
// A session may also take samples (nasr_stream_attach_audio, nasr_stream_feed_audio): a causal featurizer's
// front end (mfcc.hip: fz_stream_*) then keeps, per slot, what it needs to turn the samples of a feed into the chunk's
// stacked rows, written on the device straight into the chunk's batch slot; the forward pass over the chunk is the same.
// A look-ahead session (nasr_stream_open_lookahead) streams a bidirectional concat network: the forward
// direction's state is carried as above, the backward direction restarts in every feed R frames to the right of the rows
// the feed emits; the session holds each slot's last R feature rows on the device and a feed runs held + new rows, the
// window (lstm.hip: la_window_kernel, la_load_state_kernel, la_save_state_kernel).
#include "nasr_ctx.h"

using namespace nasr;
using namespace nasr_impl;

namespace {

int need_session(nasr_ctx* h, const char* fn) {
  if (!h->stream) return h->fail(NASR_ERR_STATE, std::string(fn) + ": no open stream session (nasr_stream_open)");
  return NASR_OK;
}

int64_t state_floats(const nasr_ctx* h) { return (int64_t)h->L * h->stream->S * 2 * h->H; }

// The chunk b (its own check first: n_frames[b] = 0 is an idle slot, and nothing is replaced when it fails): upload, the
// forward pass that continues from the session's state, the logits.
int run_chunk(nasr_ctx* h, BatchSrc b, const int32_t* n_frames, float* logits_out) {
  StreamState& ss = *h->stream;
  b.chunk = true;
  if (int rc = upload(h, b)) return rc;
  // The per-step operand images of the recurrent matrices are kept by repack() only while the per-step kernels run the
  // handle's batches; with a resident kind in use the session keeps them itself, rebuilt when the parameters have changed.
  if (h->rec_use != RecKind::Step && ss.uf_seq != h->repack_seq) {
    for (size_t k = 0; k < h->off_u.size(); ++k)
      launch_repack_u(h->P + h->off_u[k], h->Uf + k * h->Hp * h->N4, h->Ub + k * h->Hp * h->N4, h->Hp, h->st);
    ss.uf_seq = h->repack_seq;
  }
  int rc = forward(h, true);
  if (!rc) rc = fetch_logits(h, logits_out);
  // the chunk is no batch the *_resident calls could run (a slot may have no frame at all): the handle has none until the
  // next upload
  h->resident = false;
  if (rc) return rc;
  for (int s = 0; s < ss.S; ++s) ss.frames[(size_t)s] += n_frames[s];
  return NASR_OK;
}

// ---- look-ahead sessions
// What a feed does to every slot, worked out on the host from the row counts alone.
struct LaFeed {
  LaSlots sl{};
  int T = 0;      // the longest window among the slots that emit (0: no pass runs)
  int Te = 0;     // the most rows a slot emits
  int rows = 0;   // the most pending rows of any slot
  bool fresh = false;   // some slot got new rows
};

int need_lookahead(nasr_ctx* h, const char* fn) {
  if (int rc = need_session(h, fn)) return rc;
  if (!h->stream->la)
    return h->fail(NASR_ERR_STATE, std::string(fn) + ": the session has no look-ahead (nasr_stream_open_lookahead); feed it with nasr_stream_feed");
  return NASR_OK;
}

// n [S] new rows per slot (checked by the caller), last nullable.  NASR_ERR_STATE for a slot that has had `last`.
int la_plan(nasr_ctx* h, const char* fn, const int32_t* n, const uint8_t* last, LaFeed* f) {
  const StreamState& ss = *h->stream;
  const Lookahead& la = *ss.la;
  for (int b = 0; b < ss.S; ++b) {
    const bool fin = last && last[b];
    if (la.done[(size_t)b] && (n[b] > 0 || fin))
      return h->fail(NASR_ERR_STATE, std::string(fn) + ": slot " + std::to_string(b) + " has had `last`: nasr_stream_reset starts its next utterance");
    const int held = la.held[(size_t)b], P = held + n[b];
    const int E = fin ? P : std::max(0, P - la.R);
    f->sl.held[b] = held; f->sl.n[b] = n[b]; f->sl.emit[b] = E;
    if (E > 0) f->T = std::max(f->T, P);
    f->Te = std::max(f->Te, E);
    f->rows = std::max(f->rows, P);
    f->fresh |= n[b] > 0;
  }
  return NASR_OK;
}

// the host's side of a feed whose kernels are queued: rows held, slots finished, rows emitted
void la_advance(StreamState& ss, const LaFeed& f, const uint8_t* last, bool moved) {
  Lookahead& la = *ss.la;
  for (int b = 0; b < ss.S; ++b) {
    la.held[(size_t)b] = f.sl.held[b] + f.sl.n[b] - f.sl.emit[b];
    if (last && last[b]) la.done[(size_t)b] = 1;
    ss.frames[(size_t)b] += f.sl.emit[b];
  }
  if (moved) la.cur ^= 1;   // the window kernel wrote the other hold buffer
}

// The feed f: `fresh_rows` (nullable) enqueues on a stream whatever writes the new rows [S][Tc][F] into la.fresh; then the
// window assembly, and, when a slot emits, the pass over the windows and the first Te logit frames.
int run_window(nasr_ctx* h, const LaFeed& f, int Tc, const std::function<int(hipStream_t)>& fresh_rows, const uint8_t* last,
               float* logits_out) {
  StreamState& ss = *h->stream;
  Lookahead& la = *ss.la;
  HIPCHK(h, hipSetDevice(h->device));
  if (f.rows == 0 || (!f.fresh && f.Te == 0)) {        // nothing moves: only `last` on slots without rows, or all idle
    if (fresh_rows)
      if (int rc = fresh_rows(h->st)) return rc;
    la_advance(ss, f, last, false);
    return NASR_OK;
  }
  bool queued = false;
  auto assemble = [&](float* win, hipStream_t cs) -> int {
    if (fresh_rows)
      if (int rc = fresh_rows(cs)) return rc;
    launch_la_window(la.hold[la.cur].as<float>(), la.fresh.as<float>(), f.sl, win, la.hold[la.cur ^ 1].as<float>(), ss.S, la.R,
                     Tc, f.T, f.rows, h->F, cs);
    HIPCHK(h, hipGetLastError());
    queued = true;
    return NASR_OK;
  };
  if (f.T == 0) {                                      // every slot only holds: no pass, the resident batch stays
    if (int rc = assemble(nullptr, h->st)) return rc;
    la_advance(ss, f, last, true);
    return NASR_OK;
  }
  std::vector<int32_t> seq((size_t)ss.S);
  for (int b = 0; b < ss.S; ++b) seq[(size_t)b] = f.sl.emit[b] > 0 ? f.sl.held[b] + f.sl.n[b] : 0;
  StackedProducer prod;
  prod.run = assemble;
  BatchSrc b = stacked_batch(nullptr, seq.data(), nullptr, nullptr, ss.S, f.T, 0);
  b.stacked = &prod;
  b.chunk = true;
  la.sl = f.sl;
  int rc = upload(h, b);
  if (!rc) {
    if (h->rec_use != RecKind::Step && ss.uf_seq != h->repack_seq) {   // (as run_chunk)
      for (size_t k = 0; k < h->off_u.size(); ++k)
        launch_repack_u(h->P + h->off_u[k], h->Uf + k * h->Hp * h->N4, h->Ub + k * h->Hp * h->N4, h->Hp, h->st);
      ss.uf_seq = h->repack_seq;
    }
    rc = forward(h, true);
    if (!rc) rc = fetch_logits(h, logits_out, f.Te);
    h->resident = false;
  }
  if (queued) la_advance(ss, f, last, true);   // the rows have moved, whatever became of the pass
  return rc;
}

// the frame counts of a look-ahead feed: n_frames[b] in [0, Tc]
int la_check_rows(nasr_ctx* h, const char* fn, const int32_t* n, int Tc) {
  if (Tc < 0) return h->fail(NASR_ERR_ARG, std::string(fn) + ": Tc < 0");
  for (int b = 0; b < h->stream->S; ++b)
    if (n[b] < 0 || n[b] > Tc)
      return h->fail(NASR_ERR_ARG, std::string(fn) + ": n_frames[" + std::to_string(b) + "] = " + std::to_string(n[b]) +
                                       " out of [0,Tc = " + std::to_string(Tc) + "]");
  return NASR_OK;
}

}  // namespace

extern "C" {

int nasr_stream_open_lookahead(nasr_handle h, int S, int R) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  LSTM_CALL(h, "cannot stream: only the LSTM CTC networks carry state between chunks");
  if (!h->cfg.bidirectional)
    return h->fail(NASR_ERR_STATE, "nasr_stream_open_lookahead: a unidirectional network needs no look-ahead: use nasr_stream_open");
  if (h->cfg.merge != NASR_MERGE_CONCAT)
    return h->fail(NASR_ERR_STATE, "nasr_stream_open_lookahead: NASR_MERGE_STACK_RESHAPE cannot stream: its logits mix frames of the "
                                   "whole padded batch, so no chunk of it is a point in time");
  for (int i = 0; i < 4; ++i)
    if (h->cfg.dropout[i] != 0.f)
      return h->fail(NASR_ERR_STATE, "nasr_stream_open_lookahead: dropout[" + std::to_string(i) + "] = " + std::to_string(h->cfg.dropout[i]) +
                                         ": a network with dropout cannot stream (the reference applies dropout in every graph, "
                                         "keyed by the pass counter)");
  if (h->stream) return h->fail(NASR_ERR_STATE, "nasr_stream_open_lookahead: a stream session is open already");
  if (S < 1 || S > LA_MAX_SLOTS)
    return h->fail(NASR_ERR_ARG, "nasr_stream_open_lookahead: S = " + std::to_string(S) + " streams: must be in [1,64]");
  if (R < 1 || R > 1024)
    return h->fail(NASR_ERR_ARG, "nasr_stream_open_lookahead: R = " + std::to_string(R) + " look-ahead frames: must be in [1,1024]");
  HIPCHK(h, hipSetDevice(h->device));
  auto ss = std::make_unique<StreamState>();
  ss->S = S;
  ss->frames.assign((size_t)S, 0);
  ss->la = std::make_unique<Lookahead>();
  ss->la->R = R;
  ss->la->held.assign((size_t)S, 0);
  ss->la->done.assign((size_t)S, 0);
  bool grew = false;
  const size_t nb = (size_t)h->L * S * 2 * h->H * 4, hb = (size_t)S * R * h->F * 4;
  if (!ss->state.ensure(nb, &grew) || !ss->cimg.ensure((size_t)2 * rup(S, 16) * h->Hp * 4, &grew) ||
      !ss->la->hold[0].ensure(hb, &grew) || !ss->la->hold[1].ensure(hb, &grew))
    return h->fail(NASR_ERR_HIP, "nasr_stream_open_lookahead: hipMalloc of the stream state failed");
  HIPCHK(h, hipMemsetAsync(ss->state.p, 0, nb, h->st));
  h->stream = std::move(ss);
  return NASR_OK;
}

int nasr_stream_lookahead_rows(nasr_handle h, const int32_t* n_frames, const uint8_t* last, int32_t* rows_out, int* Te_out) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (int rc = need_lookahead(h, __func__)) return rc;
  if (!n_frames || !rows_out || !Te_out) return h->fail(NASR_ERR_ARG, "nasr_stream_lookahead_rows: null buffer");
  for (int b = 0; b < h->stream->S; ++b)
    if (n_frames[b] < 0)
      return h->fail(NASR_ERR_ARG, "nasr_stream_lookahead_rows: n_frames[" + std::to_string(b) + "] = " + std::to_string(n_frames[b]) + " < 0");
  LaFeed f;
  if (int rc = la_plan(h, __func__, n_frames, last, &f)) return rc;
  std::copy(f.sl.emit, f.sl.emit + h->stream->S, rows_out);
  *Te_out = f.Te;
  return NASR_OK;
}

int nasr_stream_feed_lookahead(nasr_handle h, const float* feats, const int32_t* n_frames, const uint8_t* last, int Tc,
                               int32_t* rows_out, int* Te_out, float* logits_out, int64_t logits_rows) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (int rc = need_lookahead(h, __func__)) return rc;
  StreamState& ss = *h->stream;
  if (ss.audio) return h->fail(NASR_ERR_STATE, "nasr_stream_feed_lookahead: the session takes samples (nasr_stream_feed_audio)");
  if (!n_frames || !rows_out || !Te_out) return h->fail(NASR_ERR_ARG, "nasr_stream_feed_lookahead: null buffer");
  if (int rc = la_check_rows(h, __func__, n_frames, Tc)) return rc;
  LaFeed f;
  if (int rc = la_plan(h, __func__, n_frames, last, &f)) return rc;
  if (f.fresh && !feats) return h->fail(NASR_ERR_ARG, "nasr_stream_feed_lookahead: null feats");
  if (f.Te > 0 && (!logits_out || logits_rows < f.Te))
    return h->fail(NASR_ERR_ARG, "nasr_stream_feed_lookahead: the feed emits " + std::to_string(f.Te) + " rows, logits_out holds " +
                                     std::to_string(logits_out ? logits_rows : 0) + " (nasr_stream_lookahead_rows)");
  std::copy(f.sl.emit, f.sl.emit + ss.S, rows_out);
  *Te_out = f.Te;
  std::function<int(hipStream_t)> fresh_rows;
  if (f.fresh) {
    const size_t bytes = (size_t)ss.S * Tc * h->F * 4;
    bool grew = false;
    if (!ss.la->fresh.ensure(bytes, &grew)) return h->fail(NASR_ERR_HIP, "nasr_stream_feed_lookahead: hipMalloc of the new rows failed");
    fresh_rows = [h, feats, bytes](hipStream_t cs) -> int {
      HIPCHK(h, hipMemcpyAsync(h->stream->la->fresh.p, feats, bytes, hipMemcpyHostToDevice, cs));
      return NASR_OK;
    };
  }
  return run_window(h, f, Tc, fresh_rows, last, logits_out);
}

int nasr_stream_open(nasr_handle h, int S) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  LSTM_CALL(h, "cannot stream: only the unidirectional LSTM CTC networks carry state between chunks");
  if (h->cfg.bidirectional || h->cfg.merge != NASR_MERGE_NONE)
    return h->fail(NASR_ERR_STATE, "nasr_stream_open: a bidirectional network cannot stream: its backward direction reads the "
                                   "utterance from its end");
  for (int i = 0; i < 4; ++i)
    if (h->cfg.dropout[i] != 0.f)
      return h->fail(NASR_ERR_STATE, "nasr_stream_open: dropout[" + std::to_string(i) + "] = " + std::to_string(h->cfg.dropout[i]) +
                                         ": a network with dropout cannot stream (the reference applies dropout in every graph, "
                                         "keyed by the pass counter)");
  if (h->stream) return h->fail(NASR_ERR_STATE, "nasr_stream_open: a stream session is open already");
  if (S < 1 || S > 64) return h->fail(NASR_ERR_ARG, "nasr_stream_open: S = " + std::to_string(S) + " streams: must be in [1,64]");
  HIPCHK(h, hipSetDevice(h->device));
  auto ss = std::make_unique<StreamState>();
  ss->S = S;
  ss->frames.assign((size_t)S, 0);
  bool grew = false;
  const size_t nb = (size_t)h->L * S * 2 * h->H * 4;
  if (!ss->state.ensure(nb, &grew) || !ss->cimg.ensure((size_t)rup(S, 16) * h->Hp * 4, &grew))
    return h->fail(NASR_ERR_HIP, "nasr_stream_open: hipMalloc of the stream state failed");
  HIPCHK(h, hipMemsetAsync(ss->state.p, 0, nb, h->st));
  h->stream = std::move(ss);
  return NASR_OK;
}

int nasr_stream_close(nasr_handle h) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (int rc = need_session(h, __func__)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->st));   // the last feed's kernels read the buffers that go now
  h->stream.reset();
  return NASR_OK;
}

int nasr_stream_reset(nasr_handle h, const int32_t* slots, int n) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (int rc = need_session(h, __func__)) return rc;
  StreamState& ss = *h->stream;
  HIPCHK(h, hipSetDevice(h->device));
  if (!slots) {
    HIPCHK(h, hipMemsetAsync(ss.state.p, 0, (size_t)state_floats(h) * 4, h->st));
    std::fill(ss.frames.begin(), ss.frames.end(), 0);
    if (ss.audio) fz_stream_reset(*ss.audio, -1);
    if (ss.la) {
      std::fill(ss.la->held.begin(), ss.la->held.end(), 0);
      std::fill(ss.la->done.begin(), ss.la->done.end(), 0);
    }
    return NASR_OK;
  }
  if (n < 0) return h->fail(NASR_ERR_ARG, "nasr_stream_reset: n < 0");
  for (int i = 0; i < n; ++i)
    if (slots[i] < 0 || slots[i] >= ss.S)
      return h->fail(NASR_ERR_ARG, "nasr_stream_reset: slot " + std::to_string(slots[i]) + " out of [0," + std::to_string(ss.S - 1) + "]");
  const size_t row = (size_t)2 * h->H * 4;   // one slot's (c, h) of one layer
  for (int i = 0; i < n; ++i) {
    HIPCHK(h, hipMemset2DAsync(static_cast<char*>(ss.state.p) + (size_t)slots[i] * row, (size_t)ss.S * row, 0, row, (size_t)h->L, h->st));
    ss.frames[(size_t)slots[i]] = 0;
    if (ss.audio) fz_stream_reset(*ss.audio, slots[i]);
    if (ss.la) ss.la->held[(size_t)slots[i]] = ss.la->done[(size_t)slots[i]] = 0;   // its held rows are simply forgotten
  }
  return NASR_OK;
}

int nasr_stream_feed(nasr_handle h, const float* feats, const int32_t* n_frames, int Tc, float* logits_out) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (int rc = need_session(h, __func__)) return rc;
  if (h->stream->la)
    return h->fail(NASR_ERR_STATE, "nasr_stream_feed: the session has a look-ahead: feed it with nasr_stream_feed_lookahead");
  if (!feats || !n_frames || !logits_out) return h->fail(NASR_ERR_ARG, "nasr_stream_feed: null buffer");
  return run_chunk(h, stacked_batch(feats, n_frames, nullptr, nullptr, h->stream->S, Tc, 0), n_frames, logits_out);
}

int nasr_stream_attach_audio(nasr_handle h, nasr_handle featurizer) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (int rc = need_session(h, __func__)) return rc;
  StreamState& ss = *h->stream;
  if (ss.audio) return h->fail(NASR_ERR_STATE, "nasr_stream_attach_audio: the session takes samples already");
  HIPCHK(h, hipSetDevice(h->device));
  return fz_stream_attach(h, featurizer, ss.S, &ss.audio);
}

// what the two calls below share: the session takes samples, the per-slot counts of new samples
static int audio_plan(nasr_ctx* h, const char* fn, const int64_t* nnew, const uint8_t* last, int32_t* rows_out, int* Tc_out,
                      FzFeedPlan* p) {
  if (int rc = need_session(h, fn)) return rc;
  StreamState& ss = *h->stream;
  if (!ss.audio) return h->fail(NASR_ERR_STATE, std::string(fn) + ": the session takes frames (nasr_stream_attach_audio first)");
  if (int rc = fz_stream_plan(h, *ss.audio, fn, nnew, last, p)) return rc;
  for (int b = 0; b < ss.S; ++b) rows_out[b] = (int32_t)p->slot[(size_t)b].nrows;
  *Tc_out = p->Tc;
  return NASR_OK;
}

int nasr_stream_audio_rows(nasr_handle h, const int64_t* n_samples, const uint8_t* last, int32_t* rows_out, int* Tc_out) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (!n_samples || !rows_out || !Tc_out) return h->fail(NASR_ERR_ARG, "nasr_stream_audio_rows: null buffer");
  FzFeedPlan p;
  if (int rc = audio_plan(h, __func__, n_samples, last, rows_out, Tc_out, &p)) return rc;
  if (!h->stream->la) return NASR_OK;
  LaFeed f;   // the front end's rows join the pending ones: what leaves after the look-ahead's hold-back as well
  if (int rc = la_plan(h, __func__, rows_out, last, &f)) return rc;
  std::copy(f.sl.emit, f.sl.emit + h->stream->S, rows_out);
  *Tc_out = f.Te;
  return NASR_OK;
}

// nasr_stream_feed_audio on a look-ahead session: the front end writes the feed's rows into the session's buffer of new
// rows instead of a chunk, and the window rule of nasr_stream_feed_lookahead runs on them
static int feed_audio_lookahead(nasr_ctx* h, const FzFeedPlan& p, const float* first, const uint8_t* last, int32_t* rows_out,
                                int* Tc_out, float* logits_out, int64_t logits_rows) {
  StreamState& ss = *h->stream;
  LaFeed f;
  if (int rc = la_plan(h, "nasr_stream_feed_audio", rows_out, last, &f)) return rc;
  if (f.Te > 0 && (!logits_out || logits_rows < f.Te))
    return h->fail(NASR_ERR_ARG, "nasr_stream_feed_audio: the feed emits " + std::to_string(f.Te) + " rows, logits_out holds " +
                                     std::to_string(logits_out ? logits_rows : 0) + " (nasr_stream_audio_rows)");
  std::copy(f.sl.emit, f.sl.emit + ss.S, rows_out);
  *Tc_out = f.Te;
  bool grew = false;
  if (p.Tc > 0 && !ss.la->fresh.ensure((size_t)ss.S * p.Tc * h->F * 4, &grew))
    return h->fail(NASR_ERR_HIP, "nasr_stream_feed_audio: hipMalloc of the new rows failed");
  bool ran = false;
  const int rc = run_window(h, f, p.Tc, [&](hipStream_t cs) {
    const int r = fz_stream_run(h, *ss.audio, p, first, p.Tc > 0 ? ss.la->fresh.as<float>() : nullptr, cs);
    ran = r == NASR_OK;
    return r;
  }, last, logits_out);
  if (ran) fz_stream_advance(*ss.audio, p, last);   // the front end's kernels ran, whatever became of the pass
  return rc;
}

int nasr_stream_feed_audio(nasr_handle h, const float* audio, const int64_t* offsets, const uint8_t* last, int32_t* rows_out,
                           int* Tc_out, float* logits_out, int64_t logits_rows) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (int rc = need_session(h, __func__)) return rc;
  if (!offsets || !rows_out || !Tc_out) return h->fail(NASR_ERR_ARG, "nasr_stream_feed_audio: null buffer");
  StreamState& ss = *h->stream;
  std::vector<int64_t> nnew((size_t)ss.S);
  for (int b = 0; b < ss.S; ++b) nnew[(size_t)b] = offsets[b + 1] - offsets[b];
  FzFeedPlan p;
  if (int rc = audio_plan(h, __func__, nnew.data(), last, rows_out, Tc_out, &p)) return rc;
  if (p.in_total > 0 && !audio) return h->fail(NASR_ERR_ARG, "nasr_stream_feed_audio: null audio");
  if (ss.la) return feed_audio_lookahead(h, p, p.in_total > 0 ? audio + offsets[0] : nullptr, last, rows_out, Tc_out, logits_out, logits_rows);
  if (p.Tc > 0 && (!logits_out || logits_rows < p.Tc))
    return h->fail(NASR_ERR_ARG, "nasr_stream_feed_audio: the feed emits " + std::to_string(p.Tc) + " rows, logits_out holds " +
                                     std::to_string(logits_out ? logits_rows : 0) + " (nasr_stream_audio_rows)");
  const float* first = p.in_total > 0 ? audio + offsets[0] : nullptr;
  if (p.Tc == 0) {                       // nothing to run the network on: the front end alone, the resident batch stays
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = fz_stream_run(h, *ss.audio, p, first, nullptr, h->st)) return rc;
    fz_stream_advance(*ss.audio, p, last);
    return NASR_OK;
  }
  bool queued = false;
  StackedProducer prod;
  prod.run = [&](float* dfeats, hipStream_t cs) {
    const int rc = fz_stream_run(h, *ss.audio, p, first, dfeats, cs);
    queued = rc == NASR_OK;
    return rc;
  };
  BatchSrc b = stacked_batch(nullptr, rows_out, nullptr, nullptr, ss.S, p.Tc, 0);
  b.stacked = &prod;
  const int rc = run_chunk(h, b, rows_out, logits_out);
  if (queued) fz_stream_advance(*ss.audio, p, last);   // the front end's kernels ran, whatever became of the forward pass
  return rc;
}

int nasr_stream_frames(nasr_handle h, int64_t* frames_out) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (int rc = need_session(h, __func__)) return rc;
  if (!frames_out) return h->fail(NASR_ERR_ARG, "nasr_stream_frames: null buffer");
  std::copy(h->stream->frames.begin(), h->stream->frames.end(), frames_out);
  return NASR_OK;
}

int nasr_stream_get_state(nasr_handle h, float* state, int64_t n) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (int rc = need_session(h, __func__)) return rc;
  if (!state || n != state_floats(h))
    return h->fail(NASR_ERR_ARG, "nasr_stream_get_state: expected " + std::to_string(state_floats(h)) + " floats ([L][S][2][H])");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(state, h->stream->state.p, (size_t)n * 4, hipMemcpyDeviceToHost, h->st));
  return sync_checked(h);
}

int nasr_stream_set_state(nasr_handle h, const float* state, int64_t n) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (int rc = need_session(h, __func__)) return rc;
  if (!state || n != state_floats(h))
    return h->fail(NASR_ERR_ARG, "nasr_stream_set_state: expected " + std::to_string(state_floats(h)) + " floats ([L][S][2][H])");
  if (h->stream->la)   // the held rows belong to the state they were held behind
    for (int b = 0; b < h->stream->S; ++b)
      if (h->stream->la->held[(size_t)b] > 0)
        return h->fail(NASR_ERR_STATE, "nasr_stream_set_state: slot " + std::to_string(b) + " holds " +
                                           std::to_string(h->stream->la->held[(size_t)b]) +
                                           " look-ahead rows that follow the present state: finish or reset the slot first");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(h->stream->state.p, state, (size_t)n * 4, hipMemcpyHostToDevice, h->st));
  HIPCHK(h, hipStreamSynchronize(h->st));   // the caller's array is free again
  return NASR_OK;
}

}  // extern "C"
