// nasr_stream.hip — streaming sessions on a unidirectional LSTM handle (nasr_stream_*).  The reference
// decodes whole utterances (networks/tfnetwork.py:179-181); a session keeps each stream's recurrent state (c, h) per layer
// on the device between chunks, so that a causal network recognises audio as it arrives.  A feed is an ordinary forward
// pass over the chunk (nasr_pass.hip: forward(h, true)) whose recurrence starts from the saved state and saves it again
// (lstm.hip: the state-carrying step, stream_load_state_kernel, stream_save_state_kernel).
#include "nasr_ctx.h"

using namespace nasr;
using namespace nasr_impl;

namespace {

int need_session(nasr_ctx* h, const char* fn) {
  if (!h->stream) return h->fail(NASR_ERR_STATE, std::string(fn) + ": no open stream session (nasr_stream_open)");
  return NASR_OK;
}

int64_t state_floats(const nasr_ctx* h) { return (int64_t)h->L * h->stream->S * 2 * h->H; }

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
  }
  return NASR_OK;
}

int nasr_stream_feed(nasr_handle h, const float* feats, const int32_t* n_frames, int Tc, float* logits_out) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (int rc = need_session(h, __func__)) return rc;
  if (!feats || !n_frames || !logits_out) return h->fail(NASR_ERR_ARG, "nasr_stream_feed: null buffer");
  StreamState& ss = *h->stream;
  BatchSrc b = stacked_batch(feats, n_frames, nullptr, nullptr, ss.S, Tc, 0);
  b.chunk = true;                       // its own check (n_frames[b] = 0 is an idle slot), before anything is replaced
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
