// nasr_stream.hip — streaming sessions on a unidirectional LSTM handle (nasr_stream_*).  The reference
// decodes whole utterances (networks/tfnetwork.py:179-181); a session keeps each stream's recurrent state (c, h) per layer
// on the device between chunks, so that a causal network recognises audio as it arrives.  A feed is an ordinary forward
// pass over the chunk (nasr_pass.hip: forward(h, true)) whose recurrence starts from the saved state and saves it again
// (lstm.hip: the state-carrying step, stream_load_state_kernel, stream_save_state_kernel).
// A session may also take samples (nasr_stream_attach_audio, nasr_stream_feed_audio): a causal featurizer's
// front end (mfcc.hip: fz_stream_*) then keeps, per slot, what it needs to turn the samples of a feed into the chunk's
// stacked rows, written on the device straight into the chunk's batch slot; the forward pass over the chunk is the same.
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

}  // namespace

extern "C" {

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
  }
  return NASR_OK;
}

int nasr_stream_feed(nasr_handle h, const float* feats, const int32_t* n_frames, int Tc, float* logits_out) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (int rc = need_session(h, __func__)) return rc;
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
  return audio_plan(h, __func__, n_samples, last, rows_out, Tc_out, &p);
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
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(h->stream->state.p, state, (size_t)n * 4, hipMemcpyHostToDevice, h->st));
  HIPCHK(h, hipStreamSynchronize(h->st));   // the caller's array is free again
  return NASR_OK;
}

}  // extern "C"
