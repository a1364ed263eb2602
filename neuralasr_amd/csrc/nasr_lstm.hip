// nasr_lstm.hip — the handle of the (Bi)LSTM CTC family: its set-up (lstm_create: all of nasr_create but the reading of
// the environment, which stays in nasr_api.hip, the one place that reads it), what nasr_destroy and the common calls
// need of its state (LstmState, nasr_lstm.h), and the ABI calls that only this family answers: row compaction, chunked
// training, the dropout state, the weight-gradient overlap, the deferred bucket events and the persistent recurrence's
// statistics.  Its layout and operand images are nasr_layout.hip's, its recurrence nasr_rec.hip's, its batches
// nasr_batch.hip's, its pass nasr_pass.hip's and its stream sessions nasr_stream.hip's.
#include "nasr_lstm.h"

using namespace nasr;
using namespace nasr_impl;

namespace nasr_impl {

void LstmStateDelete::operator()(LstmState* s) const { delete s; }

void drop_graphs(nasr_ctx* h) {
  if (!h->lstm) return;
  for (auto& kv : h->lstm->graphs) (void)hipGraphExecDestroy(kv.second);
  h->lstm->graphs.clear();
}

void lstm_sync_side(nasr_ctx* h) {
  if (h->lstm && h->lstm->wst) (void)hipStreamSynchronize(h->lstm->wst);
}

int lstm_logit_frames(const nasr_ctx* h, int T) {
  const nasr_model_cfg& c = h->lstm->cfg;
  return (c.bidirectional && c.merge == NASR_MERGE_STACK_RESHAPE) ? 2 * T : T;
}

int lstm_frame_skip(const nasr_ctx* h) { return h->lstm ? h->lstm->skip : 1; }

int lstm_create(const nasr_model_cfg* cfg, int device_id, void* stream, const LstmSwitches& sw, nasr_ctx** out) {
  if (!cfg || !out) {
    g_create_error = "nasr_create: null argument";
    return NASR_ERR_ARG;
  }
  *out = nullptr;
  if (cfg->feature_size < 1 || cfg->hidden < 1 || cfg->num_layers < 1 || cfg->num_classes < 2) {
    g_create_error = "nasr_create: feature_size, hidden, num_layers must be >= 1 and num_classes >= 2";
    return NASR_ERR_ARG;
  }
  if (cfg->bidirectional && cfg->merge != NASR_MERGE_STACK_RESHAPE && cfg->merge != NASR_MERGE_CONCAT) {
    g_create_error = "nasr_create: bidirectional nets need merge = STACK_RESHAPE or CONCAT";
    return NASR_ERR_ARG;
  }
  if (cfg->num_pre < 0 || cfg->num_pre > 3 || cfg->post_width < 0) {
    g_create_error = "nasr_create: num_pre must be in [0,3] and post_width >= 0";
    return NASR_ERR_ARG;
  }
  for (int i = 0; i < cfg->num_pre; ++i)
    if (cfg->pre_width[i] < 1) {
      g_create_error = "nasr_create: pre_width[i] must be >= 1 for i < num_pre";
      return NASR_ERR_ARG;
    }
  for (int i = 0; i < 4; ++i)
    if (!(cfg->dropout[i] >= 0.f && cfg->dropout[i] < 1.f)) {
      g_create_error = "nasr_create: dropout probabilities must be in [0,1)";
      return NASR_ERR_ARG;
    }
  if ((cfg->num_pre > 0 || cfg->post_width > 0) && !(cfg->relu_clip > 0.f)) {
    g_create_error = "nasr_create: relu_clip must be > 0 when dense stages are present";
    return NASR_ERR_ARG;
  }
  if ((cfg->num_pre > 0 || cfg->post_width > 0) && cfg->bidirectional && cfg->merge != NASR_MERGE_CONCAT) {
    g_create_error = "nasr_create: the DeepSpeech family concatenates the directions (merge = CONCAT)";
    return NASR_ERR_ARG;
  }
  if (cfg->bidirectional && cfg->merge == NASR_MERGE_STACK_RESHAPE && cfg->num_layers != 1) {
    g_create_error = "nasr_create: STACK_RESHAPE is the literal 1-layer BiLstmCTCNet; use CONCAT for stacks";
    return NASR_ERR_ARG;
  }
  nasr_ctx* h = nullptr;
  hipDeviceProp_t prop;
  if (int rc = handle_open("nasr_create", Family::Lstm, device_id, stream, &h, &prop)) return rc;
  h->lstm.reset(new LstmState());
  LstmState* const ls = h->lstm.get();
  ls->cfg = *cfg;
  if (!cfg->bidirectional) ls->cfg.merge = NASR_MERGE_NONE;
  h->lr = cfg->learning_rate;
  h->beta1 = cfg->beta1; h->beta2 = cfg->beta2; h->epsilon = cfg->epsilon;
  if (build_layout(h) != NASR_OK) return create_fail(h, NASR_ERR_ARG, t_err);
  ls->compactable = ls->ndense == 0 && sw.compact;
  {
    ls->sc_wr.resize(ls->L); ls->sc_wc.resize(ls->L);
    ls->sc_dr.resize(ls->ndense); ls->sc_dc.resize(ls->ndense); ls->sc_yr.resize(ls->ndense); ls->sc_yc.resize(ls->ndense);
    {
      bool ok = gemm_tph_prepare() == hipSuccess, g2 = false;
      int rmax = 1, cmax = 1;
      for (int l = 0; l < ls->L; ++l) {
        ok = ok && ls->sc_wr[l].ensure((size_t)ls->Ip[l]) && ls->sc_wc[l].ensure((size_t)ls->D * ls->N4);
        rmax = std::max(rmax, ls->Ip[l]); cmax = std::max(cmax, ls->D * ls->N4);
      }
      for (int i = 0; i < ls->ndense; ++i) {
        ok = ok && ls->sc_dr[i].ensure((size_t)ls->dIp[i]) && ls->sc_dc[i].ensure((size_t)ls->dWp[i]);
        rmax = std::max(rmax, ls->dIp[i]); cmax = std::max(cmax, ls->dWp[i]);
      }
      size_t wsf = 0;     // launch_tph_scales_batch works on all weight matrices at once
      for (int l = 0; l < ls->L; ++l) wsf += tph_scale_ws_floats(ls->Ip[l], ls->D * ls->N4);
      for (int i = 0; i < ls->ndense; ++i) wsf += tph_scale_ws_floats(ls->dIp[i], ls->dWp[i]);
      ok = ok && ls->scws.ensure(std::max(wsf, tph_scale_ws_floats(rmax, cmax)) * 4, &g2);
      if (!ok) return create_fail(h, NASR_ERR_HIP, "set-up of the fp16-plane GEMMs failed");
    }
    {
      size_t of = 0, ob = 0;
      ls->off_wftp.resize(ls->L); ls->off_wbtp.resize(ls->L);
      for (int l = 0; l < ls->L; ++l) {
        ls->off_wftp[l] = of; of += tph_bytes(ls->D * ls->N4, ls->Ip[l]);
        ls->off_wbtp[l] = ob; if (l > 0 || ls->npre > 0) ob += tph_bytes(ls->Ip[l], ls->D * ls->N4);
      }
      size_t df = 0, db = 0;
      ls->off_dftp.assign(ls->ndense, 0); ls->off_dbtp.assign(ls->ndense, 0);
      for (int i = 0; i < ls->ndense; ++i) {
        ls->off_dftp[i] = df; df += tph_bytes(ls->dWp[i], ls->dIp[i]);
        ls->off_dbtp[i] = db; if (i > 0 || ls->npre == 0) db += tph_bytes(ls->dIp[i], ls->dWp[i]);
      }
      if (hipMalloc(ls->WfTP.out(), of) != hipSuccess ||
          hipMalloc(ls->WbTP.out(), std::max<size_t>(ob, 1024)) != hipSuccess ||
          hipMalloc(ls->DfTP.out(), std::max<size_t>(df, 1024)) != hipSuccess ||
          hipMalloc(ls->DbTP.out(), std::max<size_t>(db, 1024)) != hipSuccess)
        return create_fail(h, NASR_ERR_HIP, "hipMalloc of the tiled weight planes failed");
    }
  }
  const size_t ub = (size_t)ls->L * ls->D * ls->Hp * ls->N4 * 4;
  if (!alloc_param_buffers(h) || hipMalloc(ls->Uf.out(), ub) != hipSuccess || hipMalloc(ls->Ub.out(), ub) != hipSuccess)
    return create_fail(h, NASR_ERR_HIP, "hipMalloc of parameter buffers failed");
  {
    // Buckets for an all-reduce that overlaps the rest of the backward pass (nasr_grad_bucket*): the internal layout
    // is [head | dense stages | layer 0 | ... | layer L-1 | W | b] and backward() finishes W, b first, then the layers
    // from the top down, then the dense stages in front of the stack.  Bucket 0 = layer L-1 + W + b, then one bucket
    // per layer down to layer 1, and a last one with everything in front of layer 1 INCLUDING the fault word, which
    // any launch of the step may still raise.  A one-layer net has a single bucket, unless dense stages precede it.
    ls->bucket_of_layer.assign(ls->L, -1);
    if (ls->L > 1 && ls->L <= MAX_BUCKETS) {
      for (int l = ls->L - 1; l >= 1; --l) {
        const int64_t lo = ls->off_wx[l], hi = l == ls->L - 1 ? h->np_int : ls->off_wx[l + 1];
        ls->bucket_of_layer[l] = (int)h->buckets.size();
        h->buckets.push_back({GRAD_HEAD + lo, hi - lo});
      }
      h->buckets.push_back({0, GRAD_HEAD + ls->off_wx[1]});
    } else if (ls->L == 1 && ls->npre > 0) {
      // a DeepSpeech-shaped net: the (Bi)LSTM's gradients (4/5 of the parameters at the reference's widths) + W + b are
      // complete before the backward pass of the dense stages in front of it, which then hides their all-reduce
      ls->bucket_of_layer[0] = 0;
      h->buckets.push_back({GRAD_HEAD + ls->off_wx[0], h->np_int - ls->off_wx[0]});
      h->buckets.push_back({0, GRAD_HEAD + ls->off_wx[0]});
    } else {
      h->buckets.push_back({0, GRAD_HEAD + h->np_int});
    }
  }
  (void)hipMemsetAsync(ls->Uf, 0, ub, h->st);
  (void)hipMemsetAsync(ls->Ub, 0, ub, h->st);
  if (rec_setup(h, sw.persist && prop.multiProcessorCount == 256, sw.rec_f32) != NASR_OK) return create_fail(h, NASR_ERR_HIP, t_err);
  ls->gates.resize(ls->L);
  ls->OTT.resize(ls->L);
  ls->ott_valid.assign(ls->L, 0);
  ls->outb.resize(ls->L);
  ls->cbuf.resize(ls->L);
  ls->Ybuf.resize(ls->ndense);
  ls->dYbuf.resize(ls->ndense);
  if (int rc = handle_finish(h)) return rc;
  {
    const bool eligible = ls->rec_kind == RecKind::Persist && ls->Hp == 512 && ls->L > 1;
    ls->wg_overlap = eligible && sw.wgrad_overlap;              // on unless NASR_WGRAD_OVERLAP=0 (nasr_set_wgrad_overlap)
    ls->ev_wg.resize(ls->L);
    ls->wg_pending.assign(ls->L, 0);
    if (eligible) {
      int lo = 0, hi = 0;
      (void)hipDeviceGetStreamPriorityRange(&lo, &hi);          // lo = lowest priority (largest number)
      if (hipStreamCreateWithPriority(ls->wst.out(), hipStreamNonBlocking, lo) != hipSuccess ||
          hipEventCreateWithFlags(ls->ev_dx.out(), hipEventDisableTiming) != hipSuccess)
        return create_fail(h, NASR_ERR_HIP, "set-up of the weight-gradient side stream failed");
      for (auto& e : ls->ev_wg)
        if (hipEventCreateWithFlags(e.out(), hipEventDisableTiming) != hipSuccess) return create_fail(h, NASR_ERR_HIP, "hipEventCreate failed");
      ls->bwd_lean = true;
    }
  }
  if (ls->rec_kind != RecKind::Step) ls->rearm_after = sw.rearm_after;
  if (ls->rec_kind == RecKind::Persist) ls->bucket_defer = sw.bucket_defer;
  rec_start(h);   // the census, after the weight-gradient side stream that its BPTT launch makes room for
  *out = h;
  return NASR_OK;
}

}  // namespace nasr_impl

extern "C" {

int nasr_set_row_compaction(nasr_handle h, int enabled) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  LSTM_CALL(h, "has no recurrence to compact rows for");
  // what the resident batch's plane buffers hold depends on it: takes effect with the next uploaded / committed batch
  h->lstm->compactable = enabled && h->lstm->ndense == 0;
  return NASR_OK;
}

int nasr_set_chunking(nasr_handle h, int C, int R) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  LSTM_CALL(h, "has no bidirectional recurrence to run in windows");
  LstmState* const ls = h->lstm.get();
  const std::string fn = "nasr_set_chunking";
  if (ls->stream) return h->fail(NASR_ERR_STATE, fn + ": a stream session is open: close it first");
  if (C != 0) {
    if (C < 1 || C > 4096) return h->fail(NASR_ERR_ARG, fn + ": C = " + std::to_string(C) + " chunk frames: must be in [1,4096], or 0 = off");
    if (R < 1 || R > 1024) return h->fail(NASR_ERR_ARG, fn + ": R = " + std::to_string(R) + " look-ahead frames: must be in [1,1024]");
    if (!ls->cfg.bidirectional)
      return h->fail(NASR_ERR_STATE, fn + ": a unidirectional network needs no look-ahead: its graph is causal already");
    if (ls->cfg.merge != NASR_MERGE_CONCAT)
      return h->fail(NASR_ERR_STATE, fn + ": NASR_MERGE_STACK_RESHAPE cannot stream: its logits mix frames of the whole padded batch, so "
                                          "no chunk of it is a point in time");
    for (int i = 0; i < 4; ++i)
      if (ls->cfg.dropout[i] != 0.f)
        return h->fail(NASR_ERR_STATE, fn + ": dropout[" + std::to_string(i) + "] = " + std::to_string(ls->cfg.dropout[i]) +
                                           ": a network with dropout cannot stream (the reference applies dropout in every graph, "
                                           "keyed by the pass counter)");
    if (ls->ndense)
      return h->fail(NASR_ERR_STATE, fn + ": a network with dense stages (the DeepSpeech family) is not trained in windows yet");
  }
  const int Rn = C ? R : 0;
  if (C == ls->lcC && Rn == ls->lcR) return NASR_OK;
  ls->lcC = C;
  ls->lcR = Rn;
  // the resident batch is laid out for the setting it was uploaded under: the next pass needs a new upload
  h->resident = false;
  h->have_grads = h->have_fwd = h->have_decoded = false;
  return NASR_OK;
}

int nasr_get_chunking(nasr_handle h, int* C, int* R) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (C) *C = h->lstm ? h->lstm->lcC : 0;   // (a WaveNet or LAS handle: never chunked)
  if (R) *R = h->lstm ? h->lstm->lcR : 0;
  return NASR_OK;
}

int nasr_set_frame_skip(nasr_handle h, int s) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  const std::string fn = "nasr_set_frame_skip";
  if (s < 1 || s > 8) return h->fail(NASR_ERR_ARG, fn + ": frame_skip = " + std::to_string(s) + ": must be in [1,8]");
  if (!h->lstm) {
    if (s == 1) return NASR_OK;
    return h->fail(NASR_ERR_STATE, fn + ": a WaveNet or LAS handle takes every frame (frame_skip = 1): the convolutions need each "
                                        "one, and LAS has its pyramid");
  }
  LstmState* const ls = h->lstm.get();
  if (ls->stream) return h->fail(NASR_ERR_STATE, fn + ": a stream session is open: close it first");
  if (s == ls->skip) return NASR_OK;
  ls->skip = s;
  // the resident batch is laid out for the skip it was uploaded under: the next pass needs a new upload
  h->resident = false;
  h->have_grads = h->have_fwd = h->have_decoded = false;
  return NASR_OK;
}

int nasr_get_frame_skip(nasr_handle h, int* s) {
  MODEL_CALL(h);
  if (!h || !s) return NASR_ERR_ARG;
  *s = lstm_frame_skip(h);   // (a WaveNet or LAS handle: 1)
  return NASR_OK;
}

int nasr_set_dropout_state(nasr_handle h, uint32_t seed, uint32_t counter) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  LSTM_CALL(h, "has no dropout");
  h->lstm->drop_seed = seed;
  h->lstm->drop_counter = counter;
  return NASR_OK;
}

int nasr_get_dropout_state(nasr_handle h, uint32_t* seed, uint32_t* counter) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  LSTM_CALL(h, "has no dropout");
  if (seed) *seed = h->lstm->drop_seed;
  if (counter) *counter = h->lstm->drop_counter;
  return NASR_OK;
}

int nasr_set_wgrad_overlap(nasr_handle h, int enabled) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  LSTM_CALL(h, "has no recurrence");
  LstmState* const ls = h->lstm.get();
  if (enabled && !ls->wst) return h->fail(NASR_ERR_STATE, "the weight-gradient side stream was not set up for this handle "
                                                         "(needs the persistent recurrence at Hp = 512 and more than one layer)");
  HIPCHK(h, hipStreamSynchronize(h->st));
  ls->wg_overlap = enabled != 0;
  if (h->resident) return ensure_shape(h, h->B, h->T, h->Lmax, ls->lc_live);     // the side stream's own copies of the dG planes
  return NASR_OK;
}

int nasr_get_wgrad_overlap(nasr_handle h) {
  MODEL_CALL(h);
  return h && h->lstm && h->lstm->wg_overlap ? 1 : 0;
}

int nasr_set_bucket_defer(nasr_handle h, int defer) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (h->lstm) h->lstm->bucket_defer = defer != 0;   // (a WaveNet or LAS handle: accepted, nothing to defer)
  return NASR_OK;
}

int nasr_get_persist_stats(nasr_handle h, int* aborts, int* rearms) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (aborts) *aborts = h->lstm ? h->lstm->persist_aborts : 0;   // (a WaveNet or LAS handle: no persistent recurrence)
  if (rearms) *rearms = h->lstm ? h->lstm->persist_rearms : 0;
  return NASR_OK;
}

}  // extern "C"
