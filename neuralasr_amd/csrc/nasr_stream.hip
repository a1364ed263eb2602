// nasr_stream.hip — streaming sessions on an LSTM handle (nasr_stream_*).  The reference decodes
// whole utterances (networks/tfnetwork.py:179-181); a session keeps each stream's forward recurrent state (c, h) per layer on
// the device between feeds, so that the network recognises audio as it arrives.
// One rule serves every session.  A session has a look-ahead of R frames and holds, per slot, its last rows on the device.
// With P = held + n pending rows a feed emits E = last ? P : max(0, P - R) rows: it runs an ordinary forward pass
// (nasr_pass.hip: lstm_forward(h, true)) over the pending rows of the slots that emit, the forward direction from the saved
// state (lstm.hip: load_carry_kernel, the state-carrying step), the backward direction of a bidirectional concat
// network from zero at the slot's last pending row; it saves the forward state after row E - 1
// (stream_save_state_kernel) and holds the last P - E rows (rows.hip: la_window_kernel).  A session of nasr_stream_open is the case
// R = 0 on a unidirectional network: nothing is ever held, E = n, the window is the chunk, and the state after the last
// emitted row is the state after the slot's last frame.  nasr_stream_open_lookahead opens the sessions with R >= 1.
// The rows of a feed come from the caller (nasr_stream_feed, nasr_stream_feed_lookahead) or, on a session that takes
// samples (nasr_stream_attach_audio, nasr_stream_feed_audio), from a causal featurizer's front end (nasr_fz.hip:
// fz_stream_*), which keeps per slot what it needs to turn the samples of a feed into stacked rows on the device.
// Under a frame skip (nasr_set_frame_skip) the caller's rows are input rows and everything above counts KEPT
// rows: keep_rows works out, from each slot's phase alone, which of a feed's new rows the network sees, plan_feed plans on
// those counts, and run_feed's row source passes the new rows through skip_rows_kernel (rows.hip) on their way in.
#include "nasr_fz.h"
#include "nasr_lstm.h"

using namespace nasr;
using namespace nasr_impl;

namespace {

int need_session(nasr_ctx* h, const char* fn) {
  if (!h->lstm || !h->lstm->stream) return h->fail(NASR_ERR_STATE, std::string(fn) + ": no open stream session (nasr_stream_open)");
  return NASR_OK;
}

int need_lookahead(nasr_ctx* h, const char* fn) {
  if (int rc = need_session(h, fn)) return rc;
  if (h->lstm->stream->R == 0)
    return h->fail(NASR_ERR_STATE, std::string(fn) + ": the session has no look-ahead (nasr_stream_open_lookahead); feed it with nasr_stream_feed");
  return NASR_OK;
}

int64_t state_floats(const nasr_ctx* h) { return (int64_t)h->lstm->L * h->lstm->stream->S * 2 * h->lstm->H; }

// A session of S slots and R look-ahead frames on a handle that the ABI call `fn` has found fit for it (R = 0: the
// unidirectional network's, whose call has no R to refuse).
int open_session(nasr_ctx* h, const std::string& fn, int S, int R) {
  for (int i = 0; i < 4; ++i)
    if (h->lstm->cfg.dropout[i] != 0.f)
      return h->fail(NASR_ERR_STATE, fn + ": dropout[" + std::to_string(i) + "] = " + std::to_string(h->lstm->cfg.dropout[i]) +
                                         ": a network with dropout cannot stream (the reference applies dropout in every graph, "
                                         "keyed by the pass counter)");
  if (h->lstm->stream) return h->fail(NASR_ERR_STATE, fn + ": a stream session is open already");
  if (S < 1 || S > LA_MAX_SLOTS) return h->fail(NASR_ERR_ARG, fn + ": S = " + std::to_string(S) + " streams: must be in [1,64]");
  if (h->lstm->cfg.bidirectional && (R < 1 || R > 1024))
    return h->fail(NASR_ERR_ARG, fn + ": R = " + std::to_string(R) + " look-ahead frames: must be in [1,1024]");
  HIPCHK(h, hipSetDevice(h->device));
  auto ss = std::make_unique<StreamState>();
  ss->S = S;
  ss->R = R;
  ss->frames.assign((size_t)S, 0);
  ss->held.assign((size_t)S, 0);
  ss->done.assign((size_t)S, 0);
  ss->phase.assign((size_t)S, 0);
  bool grew = false;
  const size_t nb = (size_t)h->lstm->L * S * 2 * h->lstm->H * 4, hb = (size_t)S * R * h->F * 4;
  if (!ss->state.ensure(nb, &grew) || !ss->cimg.ensure((size_t)h->lstm->D * rup(S, 16) * h->lstm->Hp * 4, &grew) ||
      (R > 0 && (!ss->hold[0].ensure(hb, &grew) || !ss->hold[1].ensure(hb, &grew))))
    return h->fail(NASR_ERR_HIP, fn + ": hipMalloc of the stream state failed");
  HIPCHK(h, hipMemsetAsync(ss->state.p, 0, nb, h->st));
  h->lstm->stream = std::move(ss);
  return NASR_OK;
}

// What a feed does to every slot, worked out on the host from the row counts alone.
struct FeedPlan {
  LaSlots sl{};         // per slot: rows held before the feed, new rows, rows emitted
  int T = 0;            // the rows of the chunk the pass runs on: the longest window among the slots that emit (0: no pass runs)
  int Te = 0;           // the logit rows fetched: the most rows a slot emits
  int rows = 0;         // the most pending rows of any slot
  bool fresh = false;   // some slot got new rows
  // the frame skip: which input rows of the feed are kept (sl.n = sk.kept), and every slot's phase behind the feed
  SkipSlots sk{};
  int phase[LA_MAX_SLOTS] = {};
};

// n_in [S] new INPUT rows per slot (checked by the caller) -> f->sk, f->phase, and kept [S], the rows of them that the
// network sees: those whose index in the slot's utterance is a multiple of the skip.  Without a skip: all of them.
// kept may be n_in itself.
void keep_rows(const nasr_ctx* h, const int32_t* n_in, FeedPlan* f, int32_t* kept) {
  const StreamState& ss = *h->lstm->stream;
  const int s = h->lstm->skip;
  for (int b = 0; b < ss.S; ++b) {
    const int n = n_in[b], ph = ss.phase[(size_t)b], first = (s - ph) % s;
    f->sk.first[b] = first;
    f->sk.kept[b] = kept[b] = n > first ? skip_frames(n - first, s) : 0;
    f->phase[b] = (int)(((int64_t)ph + n) % s);
  }
}

// n [S] new rows per slot (checked by the caller), last nullable.  NASR_ERR_STATE for a slot that has had `last`.
int plan_feed(nasr_ctx* h, const char* fn, const int32_t* n, const uint8_t* last, FeedPlan* f) {
  const StreamState& ss = *h->lstm->stream;
  for (int b = 0; b < ss.S; ++b) {
    const bool fin = last && last[b];
    if (ss.done[(size_t)b] && (n[b] > 0 || fin))
      return h->fail(NASR_ERR_STATE, std::string(fn) + ": slot " + std::to_string(b) + " has had `last`: nasr_stream_reset starts its next utterance");
    const int held = ss.held[(size_t)b], P = held + n[b];
    const int E = fin ? P : std::max(0, P - ss.R);
    f->sl.held[b] = held; f->sl.n[b] = n[b]; f->sl.emit[b] = E;
    if (E > 0) f->T = std::max(f->T, P);
    f->Te = std::max(f->Te, E);
    f->rows = std::max(f->rows, P);
    f->fresh |= n[b] > 0;
  }
  return NASR_OK;
}

// Where a feed's new rows [S][Tc][F] come from: the caller's host memory, or run(), which enqueues on stream cs whatever
// writes them, every element, to `rows` (NULL with Tc = 0: the front end only takes the samples in).  Tc counts INPUT rows:
// under a frame skip run_feed hands on [S][skip_frames(Tc, skip)][F] kept rows.
struct RowSource {
  const float* host = nullptr;
  std::function<int(float* rows, hipStream_t cs)> run;
  int Tc = 0;
};

// The feed f of ABI call `fn`: the new rows from src, and, when a slot emits, the pass over the slots' windows from the
// saved state and the first Te logit frames.  With R = 0 the new rows are the chunk: they go straight into its batch slot
// (the upload's own copy, or run() as the slot's producer).  With R > 0 they go into ss.fresh, and la_window_kernel puts
// held and new rows together into the chunk and the rows that stay held into the other hold buffer.
int run_feed(nasr_ctx* h, const char* fn, const FeedPlan& f, const RowSource& src, const uint8_t* last, float* logits_out) {
  StreamState& ss = *h->lstm->stream;
  HIPCHK(h, hipSetDevice(h->device));
  const int skip = h->lstm->skip, Tk = skip_frames(src.Tc, skip);   // Tk: the row stride of what make_rows hands on
  const size_t raw_bytes = (size_t)ss.S * src.Tc * h->F * 4, bytes = (size_t)ss.S * Tk * h->F * 4;
  float* raw = nullptr;   // skip > 1: the new input rows, all of them, before skip_rows_kernel
  if (skip > 1 && src.Tc > 0) {
    bool grew = false;
    if (!ss.raw.ensure(raw_bytes, &grew)) return h->fail(NASR_ERR_HIP, std::string(fn) + ": hipMalloc of the new rows failed");
    raw = ss.raw.as<float>();
  }
  float* fresh = nullptr;
  if (ss.R > 0 && f.fresh) {
    bool grew = false;
    if (!ss.fresh.ensure(bytes, &grew)) return h->fail(NASR_ERR_HIP, std::string(fn) + ": hipMalloc of the new rows failed");
    fresh = ss.fresh.as<float>();
  }
  bool moved = false;   // the window kernel is queued: the held rows are in the other hold buffer
  auto make_rows = [&](float* chunk, hipStream_t cs) -> int {
    float* dst = ss.R > 0 ? fresh : chunk;
    float* in = skip > 1 ? raw : dst;   // (a front end makes every input row: its running normaliser needs them all)
    if (src.run) {
      if (int rc = src.run(in, cs)) return rc;
    } else if (in && src.host) {
      HIPCHK(h, hipMemcpyAsync(in, src.host, raw_bytes, hipMemcpyHostToDevice, cs));
    }
    if (skip > 1 && in && dst) {   // into the look-ahead's new rows [S][Tk][F], or straight into the chunk [S][f.T][F]
      launch_skip_rows(in, f.sk, dst, ss.S, src.Tc, ss.R > 0 ? Tk : f.T, h->F, skip, cs);
      HIPCHK(h, hipGetLastError());
    }
    if (ss.R > 0 && (chunk || f.fresh)) {   // (neither: only `last` on slots without rows, or all idle - nothing moves)
      launch_la_window(ss.hold[ss.cur].as<float>(), fresh, f.sl, chunk, ss.hold[ss.cur ^ 1].as<float>(), ss.S, ss.R, Tk, f.T,
                       f.rows, h->F, cs);
      HIPCHK(h, hipGetLastError());
      moved = true;
    }
    return NASR_OK;
  };
  int rc;
  if (f.T == 0) {   // no slot emits: no pass, nothing is uploaded and the resident batch stays
    if ((rc = make_rows(nullptr, h->st))) return rc;
  } else {
    std::vector<int32_t> seq((size_t)ss.S);
    for (int b = 0; b < ss.S; ++b) seq[(size_t)b] = f.sl.emit[b] > 0 ? f.sl.held[b] + f.sl.n[b] : 0;
    StackedProducer prod;
    prod.run = make_rows;
    BatchSrc b = stacked_batch(ss.R == 0 && !src.run && skip == 1 ? src.host : nullptr, seq.data(), nullptr, nullptr, ss.S, f.T, 0);
    if (!b.feats) b.stacked = &prod;
    b.chunk = true;   // (its own check first: seq[b] = 0 is an idle slot, and nothing is replaced when it fails)
    ss.sl = f.sl;
    rc = upload(h, b);
    if (!rc) {
      ensure_step_images(h);   // a chunk runs on the per-step kernels, whatever the handle's kind
      rc = lstm_forward(h, true);
      if (!rc) rc = fetch_logits(h, logits_out, f.Te);
      // the chunk is no batch the *_resident calls could run (a slot may have no frame at all): the handle has none until
      // the next upload
      h->resident = false;
    }
    // Once the window kernel is queued the rows have moved, whatever became of the pass; without one (R = 0) the counts
    // follow a pass that succeeded.
    if (rc && !moved) return rc;
  }
  for (int b = 0; b < ss.S; ++b) {
    ss.held[(size_t)b] = f.sl.held[b] + f.sl.n[b] - f.sl.emit[b];
    if (last && last[b]) ss.done[(size_t)b] = 1;
    ss.frames[(size_t)b] += f.sl.emit[b];
    ss.phase[(size_t)b] = f.phase[b];
  }
  // the hold buffers alternate: shifted in place, the rows that stay held would overlap whenever fewer arrive than are held
  if (moved) ss.cur ^= 1;
  return rc;
}

// the frame counts of a look-ahead feed: n_frames[b] in [0, Tc]
int la_check_rows(nasr_ctx* h, const char* fn, const int32_t* n, int Tc) {
  if (Tc < 0) return h->fail(NASR_ERR_ARG, std::string(fn) + ": Tc < 0");
  for (int b = 0; b < h->lstm->stream->S; ++b)
    if (n[b] < 0 || n[b] > Tc)
      return h->fail(NASR_ERR_ARG, std::string(fn) + ": n_frames[" + std::to_string(b) + "] = " + std::to_string(n[b]) +
                                       " out of [0,Tc = " + std::to_string(Tc) + "]");
  return NASR_OK;
}

// the session takes samples: the front end's plan for the per-slot counts of new samples, its rows per slot
int audio_plan(nasr_ctx* h, const char* fn, const int64_t* nnew, const uint8_t* last, int32_t* rows_out, int* Tc_out, FzFeedPlan* p) {
  if (int rc = need_session(h, fn)) return rc;
  StreamState& ss = *h->lstm->stream;
  if (!ss.audio) return h->fail(NASR_ERR_STATE, std::string(fn) + ": the session takes frames (nasr_stream_attach_audio first)");
  if (int rc = fz_stream_plan(h, *ss.audio, fn, nnew, last, p)) return rc;
  for (int b = 0; b < ss.S; ++b) rows_out[b] = (int32_t)p->slot[(size_t)b].nrows;
  *Tc_out = p->Tc;
  return NASR_OK;
}

// what a planned feed reports: the rows every slot emits and the most of them
void report(const nasr_ctx* h, const FeedPlan& f, int32_t* rows_out, int* Te_out) {
  std::copy(f.sl.emit, f.sl.emit + h->lstm->stream->S, rows_out);
  *Te_out = f.Te;
}

int short_logits(nasr_ctx* h, const char* fn, const char* rows_fn, int Te, const float* logits_out, int64_t logits_rows) {
  if (Te == 0 || (logits_out && logits_rows >= Te)) return NASR_OK;
  return h->fail(NASR_ERR_ARG, std::string(fn) + ": the feed emits " + std::to_string(Te) + " rows, logits_out holds " +
                                   std::to_string(logits_out ? logits_rows : 0) + " (" + rows_fn + ")");
}

}  // namespace

extern "C" {

int nasr_stream_open(nasr_handle h, int S) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  LSTM_CALL(h, "cannot stream: only the unidirectional LSTM CTC networks carry state between chunks");
  if (h->lstm->cfg.bidirectional || h->lstm->cfg.merge != NASR_MERGE_NONE)
    return h->fail(NASR_ERR_STATE, "nasr_stream_open: a bidirectional network cannot stream: its backward direction reads the "
                                   "utterance from its end");
  return open_session(h, __func__, S, 0);
}

int nasr_stream_open_lookahead(nasr_handle h, int S, int R) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  LSTM_CALL(h, "cannot stream: only the LSTM CTC networks carry state between chunks");
  if (!h->lstm->cfg.bidirectional)
    return h->fail(NASR_ERR_STATE, "nasr_stream_open_lookahead: a unidirectional network needs no look-ahead: use nasr_stream_open");
  if (h->lstm->cfg.merge != NASR_MERGE_CONCAT)
    return h->fail(NASR_ERR_STATE, "nasr_stream_open_lookahead: NASR_MERGE_STACK_RESHAPE cannot stream: its logits mix frames of the "
                                   "whole padded batch, so no chunk of it is a point in time");
  return open_session(h, __func__, S, R);
}

int nasr_stream_close(nasr_handle h) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (int rc = need_session(h, __func__)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->st));   // the last feed's kernels read the buffers that go now
  h->lstm->stream.reset();
  return NASR_OK;
}

int nasr_stream_reset(nasr_handle h, const int32_t* slots, int n) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (int rc = need_session(h, __func__)) return rc;
  StreamState& ss = *h->lstm->stream;
  HIPCHK(h, hipSetDevice(h->device));
  if (!slots) {
    HIPCHK(h, hipMemsetAsync(ss.state.p, 0, (size_t)state_floats(h) * 4, h->st));
    std::fill(ss.frames.begin(), ss.frames.end(), 0);
    std::fill(ss.held.begin(), ss.held.end(), 0);
    std::fill(ss.done.begin(), ss.done.end(), 0);
    std::fill(ss.phase.begin(), ss.phase.end(), 0);
    if (ss.audio) fz_stream_reset(*ss.audio, -1);
    return NASR_OK;
  }
  if (n < 0) return h->fail(NASR_ERR_ARG, "nasr_stream_reset: n < 0");
  for (int i = 0; i < n; ++i)
    if (slots[i] < 0 || slots[i] >= ss.S)
      return h->fail(NASR_ERR_ARG, "nasr_stream_reset: slot " + std::to_string(slots[i]) + " out of [0," + std::to_string(ss.S - 1) + "]");
  const size_t row = (size_t)2 * h->lstm->H * 4;   // one slot's (c, h) of one layer
  for (int i = 0; i < n; ++i) {
    HIPCHK(h, hipMemset2DAsync(static_cast<char*>(ss.state.p) + (size_t)slots[i] * row, (size_t)ss.S * row, 0, row, (size_t)h->lstm->L, h->st));
    ss.frames[(size_t)slots[i]] = 0;
    ss.held[(size_t)slots[i]] = ss.done[(size_t)slots[i]] = 0;   // its held rows are simply forgotten
    ss.phase[(size_t)slots[i]] = 0;
    if (ss.audio) fz_stream_reset(*ss.audio, slots[i]);
  }
  return NASR_OK;
}

int nasr_stream_feed(nasr_handle h, const float* feats, const int32_t* n_frames, int Tc, float* logits_out) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (int rc = need_session(h, __func__)) return rc;
  if (h->lstm->stream->R > 0)
    return h->fail(NASR_ERR_STATE, "nasr_stream_feed: the session has a look-ahead: feed it with nasr_stream_feed_lookahead");
  if (!feats || !n_frames || !logits_out) return h->fail(NASR_ERR_ARG, "nasr_stream_feed: null buffer");
  if (int rc = validate_chunk(h, n_frames, h->lstm->stream->S, Tc)) return rc;
  FeedPlan f;
  std::vector<int32_t> kept((size_t)h->lstm->stream->S);
  keep_rows(h, n_frames, &f, kept.data());
  if (int rc = plan_feed(h, __func__, kept.data(), nullptr, &f)) return rc;
  // The chunk is the caller's, Tc rows (skip_frames(Tc, skip) of them kept) and not the longest slot's: its row count
  // decides how the bulk GEMMs split their sums.  So a chunk in which every slot is idle runs as well, and replaces the
  // resident batch.
  f.T = f.Te = skip_frames(Tc, h->lstm->skip);
  RowSource src;
  src.host = feats;
  src.Tc = Tc;
  return run_feed(h, __func__, f, src, nullptr, logits_out);
}

int nasr_stream_lookahead_rows(nasr_handle h, const int32_t* n_frames, const uint8_t* last, int32_t* rows_out, int* Te_out) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (int rc = need_lookahead(h, __func__)) return rc;
  if (!n_frames || !rows_out || !Te_out) return h->fail(NASR_ERR_ARG, "nasr_stream_lookahead_rows: null buffer");
  for (int b = 0; b < h->lstm->stream->S; ++b)
    if (n_frames[b] < 0)
      return h->fail(NASR_ERR_ARG, "nasr_stream_lookahead_rows: n_frames[" + std::to_string(b) + "] = " + std::to_string(n_frames[b]) + " < 0");
  FeedPlan f;
  std::vector<int32_t> kept((size_t)h->lstm->stream->S);
  keep_rows(h, n_frames, &f, kept.data());
  if (int rc = plan_feed(h, __func__, kept.data(), last, &f)) return rc;
  report(h, f, rows_out, Te_out);
  return NASR_OK;
}

int nasr_stream_feed_lookahead(nasr_handle h, const float* feats, const int32_t* n_frames, const uint8_t* last, int Tc,
                               int32_t* rows_out, int* Te_out, float* logits_out, int64_t logits_rows) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (int rc = need_lookahead(h, __func__)) return rc;
  if (h->lstm->stream->audio) return h->fail(NASR_ERR_STATE, "nasr_stream_feed_lookahead: the session takes samples (nasr_stream_feed_audio)");
  if (!n_frames || !rows_out || !Te_out) return h->fail(NASR_ERR_ARG, "nasr_stream_feed_lookahead: null buffer");
  if (int rc = la_check_rows(h, __func__, n_frames, Tc)) return rc;
  FeedPlan f;
  std::vector<int32_t> kept((size_t)h->lstm->stream->S);
  keep_rows(h, n_frames, &f, kept.data());
  if (int rc = plan_feed(h, __func__, kept.data(), last, &f)) return rc;
  if (f.fresh && !feats) return h->fail(NASR_ERR_ARG, "nasr_stream_feed_lookahead: null feats");
  if (int rc = short_logits(h, __func__, "nasr_stream_lookahead_rows", f.Te, logits_out, logits_rows)) return rc;
  report(h, f, rows_out, Te_out);
  RowSource src;
  src.host = feats;
  src.Tc = Tc;
  return run_feed(h, __func__, f, src, last, logits_out);
}

int nasr_stream_attach_audio(nasr_handle h, nasr_handle featurizer) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (int rc = need_session(h, __func__)) return rc;
  StreamState& ss = *h->lstm->stream;
  if (ss.audio) return h->fail(NASR_ERR_STATE, "nasr_stream_attach_audio: the session takes samples already");
  HIPCHK(h, hipSetDevice(h->device));
  return fz_stream_attach(h, featurizer, ss.S, &ss.audio);
}

int nasr_stream_audio_rows(nasr_handle h, const int64_t* n_samples, const uint8_t* last, int32_t* rows_out, int* Tc_out) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (!n_samples || !rows_out || !Tc_out) return h->fail(NASR_ERR_ARG, "nasr_stream_audio_rows: null buffer");
  FzFeedPlan p;
  if (int rc = audio_plan(h, __func__, n_samples, last, rows_out, Tc_out, &p)) return rc;
  FeedPlan f;   // the front end's rows, those the frame skip keeps, join the pending ones: what leaves after the look-ahead's hold-back
  keep_rows(h, rows_out, &f, rows_out);
  if (int rc = plan_feed(h, __func__, rows_out, last, &f)) return rc;
  report(h, f, rows_out, Tc_out);
  return NASR_OK;
}

int nasr_stream_feed_audio(nasr_handle h, const float* audio, const int64_t* offsets, const uint8_t* last, int32_t* rows_out,
                           int* Tc_out, float* logits_out, int64_t logits_rows) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (int rc = need_session(h, __func__)) return rc;
  if (!offsets || !rows_out || !Tc_out) return h->fail(NASR_ERR_ARG, "nasr_stream_feed_audio: null buffer");
  StreamState& ss = *h->lstm->stream;
  std::vector<int64_t> nnew((size_t)ss.S);
  for (int b = 0; b < ss.S; ++b) nnew[(size_t)b] = offsets[b + 1] - offsets[b];
  FzFeedPlan p;
  if (int rc = audio_plan(h, __func__, nnew.data(), last, rows_out, Tc_out, &p)) return rc;
  if (p.in_total > 0 && !audio) return h->fail(NASR_ERR_ARG, "nasr_stream_feed_audio: null audio");
  FeedPlan f;
  keep_rows(h, rows_out, &f, rows_out);
  if (int rc = plan_feed(h, __func__, rows_out, last, &f)) return rc;
  if (int rc = short_logits(h, __func__, "nasr_stream_audio_rows", f.Te, logits_out, logits_rows)) return rc;
  report(h, f, rows_out, Tc_out);
  const float* first = p.in_total > 0 ? audio + offsets[0] : nullptr;
  bool ran = false;
  RowSource src;
  src.Tc = p.Tc;
  src.run = [&](float* rows, hipStream_t cs) {
    const int rc = fz_stream_run(h, *ss.audio, p, first, rows, cs);
    ran = rc == NASR_OK;
    return rc;
  };
  const int rc = run_feed(h, __func__, f, src, last, logits_out);
  if (ran) fz_stream_advance(*ss.audio, p, last);   // the front end's kernels ran, whatever became of the pass
  return rc;
}

int nasr_stream_frames(nasr_handle h, int64_t* frames_out) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (int rc = need_session(h, __func__)) return rc;
  if (!frames_out) return h->fail(NASR_ERR_ARG, "nasr_stream_frames: null buffer");
  std::copy(h->lstm->stream->frames.begin(), h->lstm->stream->frames.end(), frames_out);
  return NASR_OK;
}

int nasr_stream_get_state(nasr_handle h, float* state, int64_t n) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (int rc = need_session(h, __func__)) return rc;
  if (!state || n != state_floats(h))
    return h->fail(NASR_ERR_ARG, "nasr_stream_get_state: expected " + std::to_string(state_floats(h)) + " floats ([L][S][2][H])");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(state, h->lstm->stream->state.p, (size_t)n * 4, hipMemcpyDeviceToHost, h->st));
  return sync_checked(h);
}

int nasr_stream_set_state(nasr_handle h, const float* state, int64_t n) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (int rc = need_session(h, __func__)) return rc;
  if (!state || n != state_floats(h))
    return h->fail(NASR_ERR_ARG, "nasr_stream_set_state: expected " + std::to_string(state_floats(h)) + " floats ([L][S][2][H])");
  for (int b = 0; b < h->lstm->stream->S; ++b)   // the held rows belong to the state they were held behind
    if (h->lstm->stream->held[(size_t)b] > 0)
      return h->fail(NASR_ERR_STATE, "nasr_stream_set_state: slot " + std::to_string(b) + " holds " +
                                         std::to_string(h->lstm->stream->held[(size_t)b]) +
                                         " look-ahead rows that follow the present state: finish or reset the slot first");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(h->lstm->stream->state.p, state, (size_t)n * 4, hipMemcpyHostToDevice, h->st));
  HIPCHK(h, hipStreamSynchronize(h->st));   // the caller's array is free again
  std::fill(h->lstm->stream->phase.begin(), h->lstm->stream->phase.end(), 0);   // the state carries no frame-skip phase
  return NASR_OK;
}

}  // extern "C"
