// nasr_pass.hip — one step on the handle's streams: forward pass (dense stages, hoisted input GEMMs, recurrence, projection),
// CTC, backward pass (projection, BPTT, input / weight gradients, gradient buckets).  The graph of create_network
// (networks/bilstm_ctc_net.py:10-52, networks/lstm_ctc_net.py:10-47, networks/deepspeech.py:43-121) and its gradients
// (networks/tfnetwork.py:115-140) as launches; see DESIGN.md §4.
#include "nasr_lstm.h"

using namespace nasr;
using namespace nasr_impl;

namespace nasr_impl {

// ---- the per-step kernels' view of layer l (StepWindow, kernels.h): T steps over the layer's buffers from row `row` on,
// with seq as their seq_len; c0: the carried c of a window that continues a sequence, or NULL
static StepWindow step_window(nasr_ctx* h, int l, int T, size_t row, const int* seq, const float* c0) {
  LstmState* const ls = h->lstm.get();
  const size_t sU = (size_t)l * ls->D * ls->Hp * ls->N4, DH = (size_t)ls->D * ls->Hp, DN = (size_t)ls->D * ls->N4;
  StepWindow w{};
  w.dm = {T, h->B, h->Bp, ls->H, ls->Hp, ls->D};
  w.Uf = ls->Uf + sU; w.Ub = ls->Ub + sU;
  w.hstate = ls->hstate.as<float>(); w.partial = ls->partial.as<float>(); w.dcstate = ls->dcstate.as<float>();
  w.gates = ls->gates[l].as<float>() + row * DN; w.cbuf = ls->cbuf[l].as<float>() + row * DH; w.out = ls->outb[l].as<float>() + row * DH;
  w.dg = dg_of(ls, l) + row * DN; w.dout = dout_of(ls, l) + row * DH;
  w.seq_len = seq; w.forget_bias = ls->cfg.forget_bias; w.c0 = c0;
  return w;
}

// ---- one layer pass of the recurrence: the whole pass in the resident kind in use (nasr_rec.hip), or the per-timestep
// launches of the batch's T steps, optionally replayed from a hipGraph.  *launches += the recurrence launches it enqueued.
static int run_steps(nasr_ctx* h, int l, bool bwd, hipStream_t st, int* launches) {
  LstmState* const ls = h->lstm.get();
  if (ls->rec_use != RecKind::Step) return rec_launch(h, l, bwd, st, launches);
  *launches += h->T;
  const StepWindow w = step_window(h, l, h->T, 0, h->seq_p, nullptr);
  auto body = [&]() { bwd ? lstm_steps_bwd(w, 0, h->T, st) : lstm_steps_fwd(w, 0, h->T, st); };
  if (!h->graph_mode) {
    body();
    HIPCHK(h, hipGetLastError());
    return NASR_OK;
  }
  const GraphKey key{h->T, l, bwd ? 1 : 0};
  auto it = ls->graphs.find(key);
  if (it == ls->graphs.end()) {
    if (ls->graphs.size() > 256) drop_graphs(h);
    hipGraph_t g = nullptr;
    HIPCHK(h, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    body();
    HIPCHK(h, hipStreamEndCapture(st, &g));
    hipGraphExec_t ex = nullptr;
    HIPCHK(h, hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
    (void)hipGraphDestroy(g);
    it = ls->graphs.emplace(key, ex).first;
  }
  HIPCHK(h, hipGraphLaunch(it->second, st));
  return NASR_OK;
}

// The same over the windows of a chunked batch (ls->lc_live).  Window k of layer l is rows [k*W, (k+1)*W) of
// the layer's buffers with wlen[k] as its seq_len: to the step kernels a batch of W frames that continues from the carried
// state.  No graph, as a stream feed has none: step 0 is another kernel than the rest.
int lc_run_steps(nasr_ctx* h, int l, bool bwd, hipStream_t st, int* launches) {
  LstmState* const ls = h->lstm.get();
  const LcGeom& g = ls->lcg;
  const int Bp = h->Bp, Hp = ls->Hp, D = ls->D, W = g.W, DH = D * Hp;
  const int Ce = std::min(g.C, W);                   // W <= C: the one window of a batch no longer than a chunk
  float *cimg = ls->lc_cimg.as<float>(), *dcc = ls->lc_dcc.as<float>();
  float *cb = ls->cbuf[l].as<float>(), *ob = ls->outb[l].as<float>();
  for (int i = 0; i < g.K; ++i) {
    const int k = bwd ? g.K - 1 - i : i;
    const int* wl = h->wlen_p + (size_t)k * Bp;
    const StepWindow w = step_window(h, l, W, (size_t)k * W * Bp, wl, cimg);
    if (!bwd) {
      launch_lc_load_carry(ob, cb, h->wlen_p, k, g, w.hstate, cimg, Hp, D, st);
      lstm_steps_fwd(w, 0, W, st);
      continue;
    }
    lstm_steps_bwd(w, Ce, W, st);
    // the forward state after step C-1 went on into window k+1: so does its dc come back (that window's BPTT left it in
    // dcc), into the chain at the step that reads it
    if (k + 1 < g.K) launch_lc_carry_dc(lstm_steps_dcin(w, Ce - 1), dcc, Bp * Hp, st);
    lstm_steps_bwd(w, 1, Ce, st);
    launch_lc_load_carry(ob, cb, h->wlen_p, k, g, w.hstate, cimg, Hp, D, st);   // (hstate: free during BPTT; only cimg is read)
    lstm_steps_bwd(w, 0, 1, st);                     // step 0, in the carry form
    const StepLeft left = lstm_steps_left(w, 0);     // what step 0 left: the gradient with respect to the carried (h, c)
    if (k > 0)
      launch_lc_carry_out(left.partial, lstm_bwd_partials(Hp), left.dc, wl, dout_of(ls, l) + ((size_t)(k - 1) * W + g.C - 1) * Bp * DH,
                          dcc, Bp, Hp, DH, st);
  }
  *launches += g.K * W;
  HIPCHK(h, hipGetLastError());
  return NASR_OK;
}

float* ensure_slabs(nasr_ctx* h, int split, int M, int N) {
  if (split <= 1) return nullptr;
  bool grew = false;
  if (!h->slabs.ensure((size_t)split * M * N * 4, &grew)) return nullptr;
  return h->slabs.as<float>();
}

int gemm_f32(nasr_ctx* h, GemmDesc g) {
  g.slabs = ensure_slabs(h, g.split_k, g.M, g.N);
  if (g.split_k > 1 && !g.slabs) return h->fail(NASR_ERR_HIP, "slab workspace allocation failed");
  launch_gemm(g, h->st);
  HIPCHK(h, hipGetLastError());
  return NASR_OK;
}

int gemm_dense(nasr_ctx* h, const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc, bool a_col,
               bool b_col, const float* bias, int a_shift, int a_rows) {
  GemmDesc g{};
  g.A = A; g.B = B; g.C = C;
  g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc;
  g.a_col = a_col; g.b_col = b_col;
  g.a_shift = a_shift;
  g.a_rows = a_rows >= 0 ? a_rows : (a_col ? K : M);
  g.bias = bias;
  g.split_k = bias ? 1 : gemm_pick_split(M, N, K);
  return gemm_f32(h, g);
}

// operand scales of layer l's dG (rows = frames: sc_gr, optional; columns = gates: sc_gc): from the maxima the persistent
// BPTT kernel took while it stored dG, or by a pass over dG
void dg_scales(nasr_ctx* h, int l, int R, bool rows, hipStream_t st) {
  LstmState* const ls = h->lstm.get();
  const int DN = ls->D * ls->N4;
  if (ls->dgmax_layer == l) {
    const float* rp = ls->dgmax.as<float>();
    launch_tph_scales_from_parts(rp, ls->D * 32, R, rows ? ls->sc_gr.sp() : nullptr, rows ? ls->sc_gr.ip() : nullptr,
                                 rp + (size_t)ls->D * 32 * R, 8 / ls->D, DN, gc_of(ls, l).sp(), gc_of(ls, l).ip(), st);
  } else {
    pl_scales(h, dg_of(ls, l), R, DN, DN, rows ? &ls->sc_gr : nullptr, &gc_of(ls, l), st);
  }
}

// gates_l = X_l * Wx_l + bias_l over all R rows - or, for a ragged batch (h->cmp_rows, nasr_ctx.h), over its frames only:
// the split pass gathers them, the epilogue scatters the result rows back (padding rows of gates_l keep what they had; the
// recurrence kernels select by t < seq_len[b] and never use them)
void gemm_xproj(nasr_ctx* h, int l, int R, hipStream_t st) {
  LstmState* const ls = h->lstm.get();
  const int D = ls->D, N4 = ls->N4, Ip = ls->Ip[l];
  const int rows = h->cmp_rows ? h->cmp_rows : R;
  const int* vm = h->cmp_rows ? h->vrow_p : nullptr;
  ActScale as = lstm_in_scale(ls, l);
  if (vm && l == 0) { as.rs = ls->sc_cx.sp(); as.rinv = ls->sc_cx.ip(); }   // the feature rows' scales in the compacted order
  // a training step wants the layer below's output a second time, with the frame index as contraction index (its own
  // recurrent weight gradient and this layer's input weight gradient): both plane sets in this one pass over it
  const bool both = l > 0 && h->cur && h->cur->has_labels;
  launch_tph_split2(lstm_input(h, l), ls->XTP.as<unsigned char>(), both ? ls->OTT[l - 1].as<unsigned char>() : nullptr, rows, Ip, Ip,
                    as.rs, 1.f, both ? as.cs : nullptr, 1.f, nullptr, st, vm);
  if (l > 0) ls->ott_valid[l - 1] = both;
  GemmTPHDesc g{};
  g.A = ls->XTP.as<unsigned char>(); g.B = ls->WfTP + ls->off_wftp[l]; g.C = ls->gates[l].as<float>();
  g.M = rows; g.N = D * N4; g.K = Ip; g.nkbA = (Ip + 15) / 16; g.nkbB = g.nkbA; g.ldc = D * N4;
  g.bias = h->P + ls->off_bias[l]; g.split_k = 1;
  g.c_map = vm;
  pl_gemm(g, as.rinv, ls->sc_wc[l].ip(), st);
}

// dOut_{l-1} = dG_l * Wx_l^T : the gradient wrt layer l's input = the layer below's output.  weight_grads(l) follows:
// dG is split ONCE into both plane sets (frame-row scales for this product, gate-column scales for the weight gradients)
// and its 64-row partial column sums (the bias gradient).  (Ragged batch: over the compacted rows, as gemm_xproj.)
void gemm_dx(nasr_ctx* h, int l, int R, hipStream_t st) {
  LstmState* const ls = h->lstm.get();
  const int D = ls->D, N4 = ls->N4;
  const int rows = h->cmp_rows ? h->cmp_rows : R;
  const int* vm = h->cmp_rows ? h->vrow_p : nullptr;
  const float* A = dg_of(ls, l);
  float* C = l > 0 ? dout_of(ls, l - 1) : ls->dYbuf[ls->npre - 1].as<float>();
  dg_scales(h, l, R, true, st);
  const float *rs = ls->sc_gr.sp(), *rinv = ls->sc_gr.ip();
  if (vm) {
    launch_gather_rows(ls->sc_cr.sp(), ls->sc_gr.sp(), vm, h->cmp_rows_p, 1.f, st);
    launch_gather_rows(ls->sc_cr.ip(), ls->sc_gr.ip(), vm, h->cmp_rows_p, 1.f, st);
    rs = ls->sc_cr.sp(); rinv = ls->sc_cr.ip();
  }
  launch_tph_split2(A, ls->GTP.as<unsigned char>(), gttp_of(ls, l), rows, D * N4, D * N4, rs, 1.f, gc_of(ls, l).sp(), 1.f,
                    csws_of(ls, l), st, vm);
  ls->gttp_layer = l;   // weight_grads(l): transposed planes and column-sum partials of dG are there
  GemmTPHDesc g{};
  g.A = ls->GTP.as<unsigned char>(); g.B = ls->WbTP + ls->off_wbtp[l]; g.C = C;
  g.M = rows; g.N = ls->Ip[l]; g.K = D * N4; g.nkbA = (D * N4 + 15) / 16; g.nkbB = g.nkbA; g.ldc = ls->Ip[l];
  g.split_k = gemm_tph_pick_split(g.M, g.N, g.K);
  g.slabs = ensure_slabs(h, g.split_k, g.M, g.N);
  if (g.split_k > 1 && !g.slabs) g.split_k = 1;
  g.c_map = vm;
  pl_gemm(g, rinv, ls->sc_wr[l].ip(), st);
}

// ---- dense stages (networks/deepspeech.py:43-68,106-113) -----------------------------------------------------
// Y_i = dropout(min(relu(X W_i + b_i), clip)): one tiled-plane GEMM + the in-place epilogue of dense.hip
int dense_forward(nasr_ctx* h, int i, const float* X) {
  LstmState* const ls = h->lstm.get();
  const int R = h->T * h->Bp, Ip = ls->dIp[i], Wp = ls->dWp[i];
  const ActScale as = dense_in_scale(ls, i);
  pl_split(X, ls->XTP.as<unsigned char>(), nullptr, R, Ip, Ip, as.rs, nullptr, nullptr, h->st);
  GemmTPHDesc g{};
  g.A = ls->XTP.as<unsigned char>(); g.B = ls->DfTP + ls->off_dftp[i]; g.C = ls->Ybuf[i].as<float>();
  g.M = R; g.N = Wp; g.K = Ip; g.nkbA = (Ip + 15) / 16; g.nkbB = g.nkbA; g.ldc = Wp;
  g.bias = h->P + ls->off_db[i]; g.split_k = 1;
  pl_gemm(g, as.rinv, ls->sc_dc[i].ip(), h->st);
  launch_dense_act(ls->Ybuf[i].as<float>(), R, h->Bp, h->B, ls->dWid[i], Wp, ls->cfg.relu_clip, ls->cfg.dropout[i],
                   ls->drop_seed, ls->drop_counter, i, h->st);
  // the stage's output feeds the next GEMM (rows = frames) and, transposed, its weight gradient (rows = features)
  pl_scales(h, ls->Ybuf[i].as<float>(), R, Wp, Wp, &ls->sc_yr[i], &ls->sc_yc[i], h->st);
  HIPCHK(h, hipGetLastError());
  return NASR_OK;
}

// dY_i (in dYbuf[i]) -> dW_i, db_i and, when dX is given, the gradient wrt the stage's input [R][dIp]
int dense_backward(nasr_ctx* h, int i, const float* X, float* dX) {
  LstmState* const ls = h->lstm.get();
  const int R = h->T * h->Bp, Ip = ls->dIp[i], Wp = ls->dWp[i];
  const int nkb = (R + 15) / 16;
  float* dZ = ls->dYbuf[i].as<float>();
  launch_dense_act_bwd(dZ, ls->Ybuf[i].as<float>(), (int64_t)R * Wp, ls->cfg.relu_clip, ls->cfg.dropout[i], h->st);
  const ActScale as = dense_in_scale(ls, i);
  pl_scales(h, dZ, R, Wp, Wp, dX ? &ls->sc_gr : nullptr, &ls->sc_gc, h->st);
  // both forms of dZ (the first only when an input gradient follows) + column-sum partials in one pass
  pl_split(dZ, dX ? ls->GTP.as<unsigned char>() : nullptr, ls->GTTP.as<unsigned char>(), R, Wp, Wp, ls->sc_gr.sp(),
           ls->sc_gc.sp(), ls->csws.as<float>(), h->st);
  pl_split(X, nullptr, ls->DTP.as<unsigned char>(), R, Ip, Ip, nullptr, as.cs, nullptr, h->st);
  {  // dW = X^T dZ
    GemmTPHDesc g{};
    g.A = ls->DTP.as<unsigned char>(); g.B = ls->GTTP.as<unsigned char>(); g.C = h->G + ls->off_dw[i];
    g.M = Ip; g.N = Wp; g.K = R; g.nkbA = nkb; g.nkbB = nkb; g.ldc = Wp;
    g.split_k = gemm_tph_pick_split(g.M, g.N, g.K);
    g.slabs = ensure_slabs(h, g.split_k, g.M, g.N);
    if (g.split_k > 1 && !g.slabs) return h->fail(NASR_ERR_HIP, "slab workspace allocation failed");
    pl_gemm(g, as.cinv, ls->sc_gc.ip(), h->st);
  }
  launch_colsum_parts(ls->csws.as<float>(), tp_split2_parts(R), Wp, h->G + ls->off_db[i], h->st);
  if (dX) {  // dX = dZ W^T
    GemmTPHDesc g{};
    g.A = ls->GTP.as<unsigned char>(); g.B = ls->DbTP + ls->off_dbtp[i]; g.C = dX;
    g.M = R; g.N = Ip; g.K = Wp; g.nkbA = (Wp + 15) / 16; g.nkbB = g.nkbA; g.ldc = Ip;
    g.split_k = gemm_tph_pick_split(g.M, g.N, g.K);
    g.slabs = ensure_slabs(h, g.split_k, g.M, g.N);
    if (g.split_k > 1 && !g.slabs) g.split_k = 1;
    pl_gemm(g, ls->sc_gr.ip(), ls->sc_dr[i].ip(), h->st);
  }
  HIPCHK(h, hipGetLastError());
  return NASR_OK;
}

// One layer of a stream chunk: the recurrence over the chunk's T steps on the per-step kernels, whatever kind the handle's
// batches run on: the forward direction from the session's saved (c, h) of layer l, a backward direction (a look-ahead
// session's) from zero at each slot's last pending row (seq_len[b] = its window).  Saved again is the forward state after
// every slot's last emitted row; without a look-ahead that is its last frame.  No graph: step 0 is another kernel than
// the rest, and a chunk is a few dozen launches.
static int run_chunk_steps(nasr_ctx* h, int l, hipStream_t st) {
  LstmState* const ls = h->lstm.get();
  StreamState& ss = *ls->stream;
  float* state = ss.state.as<float>() + (size_t)l * ss.S * 2 * ls->H;
  const StepWindow w = step_window(h, l, h->T, 0, h->seq_p, ss.cimg.as<float>());
  launch_stream_load_state(state, w.hstate, ss.cimg.as<float>(), ss.S, ls->H, h->Bp, ls->Hp, st, ls->D);
  lstm_steps_fwd(w, 0, h->T, st);
  launch_stream_save_state(w.out, w.cbuf, ss.sl, state, ss.S, ls->H, h->Bp, ls->D * ls->Hp, st);
  h->n_fwd_launch += h->T;
  HIPCHK(h, hipGetLastError());
  return NASR_OK;
}

int forward(nasr_ctx* h) {
  if (!h->resident) return h->fail(NASR_ERR_STATE, "no resident batch: call nasr_upload_batch first");
  switch (h->family) {
    case Family::WaveNet: return wn_forward(h, false);   // forward-only calls: inference-mode batch norm
    case Family::Las: return h->fail(NASR_ERR_STATE, "a LAS handle has no CTC logits: use nasr_las_forward");
    default: return lstm_forward(h);
  }
}

int lstm_forward(nasr_ctx* h, bool chunk) {
  LstmState* const ls = h->lstm.get();
  const int Bp = h->Bp, T = h->T, D = ls->D, Hp = ls->Hp;
  const int R = T * Bp, Rv = ls->Tv * Bp;   // rows by frame; rows of the LSTM stack (the same but for a chunked batch)
  const bool lc = ls->lc_live;
  if (lc) ensure_step_images(h);   // a chunked batch runs on the per-step kernels, whatever the handle's kind
  h->n_fwd_launch = 0;
  std::fill(ls->ott_valid.begin(), ls->ott_valid.end(), 0);
  // the fault word of the pass that starts here (a training step or a forward-only call); what an unread earlier word
  // said is gone with it
  if (!chunk) HIPCHK(h, hipMemsetAsync(h->Gbase, 0, GRAD_HEAD * 4, h->st));
  // the control blocks of this pass's persistent launches, cleared in one go (one per layer: run_steps)
  if (ls->rec_use == RecKind::Persist && !chunk && !lc) {
    HIPCHK(h, hipMemsetAsync(ls->pctl + 1, 0, (size_t)ls->L * sizeof(PersistCtl), h->st));
    HIPCHK(h, hipMemsetAsync(ls->xchf, 0, (size_t)ls->L * persist_hx_bytes(ls->Hp), h->st));   // epoch 0 everywhere (lstm_persist.hip)
  }
  for (int i = 0; i < ls->npre; ++i) {
    PhaseScope ps(h, PH_XPROJ);
    int rc = dense_forward(h, i, i == 0 ? h->X0.as<float>() : ls->Ybuf[i - 1].as<float>());
    if (rc) return rc;
  }
  for (int l = 0; l < ls->L; ++l) {
    {
      PhaseScope ps(h, PH_XPROJ);
      gemm_xproj(h, l, Rv, h->st);
      HIPCHK(h, hipGetLastError());
    }
    PhaseScope ps(h, PH_RECF);
    int rc = chunk ? run_chunk_steps(h, l, h->st)
             : lc  ? lc_run_steps(h, l, false, h->st, &h->n_fwd_launch)
                   : run_steps(h, l, false, h->st, &h->n_fwd_launch);
    if (rc) return rc;
  }
  if (lc) {   // the rows the windows emit, by frame: what the projection, and everything behind it, reads
    PhaseScope ps(h, PH_RECF);
    launch_lc_emit(ls->outb[ls->L - 1].as<float>(), h->seq_p, ls->lc_top.as<float>(), ls->lcg, D * Hp, h->st);
  }
  if (ls->has_post) {
    PhaseScope ps(h, PH_XPROJ);
    int rc = dense_forward(h, ls->npre, ls->outb[ls->L - 1].as<float>());
    if (rc) return rc;
  }
  if (ls->ndense && !chunk) ls->drop_counter += 1;   // one counter value per forward pass (a chunk: no dropout, no count)
  {
    PhaseScope ps(h, PH_PROJCTC);
    const bool sr = ls->cfg.merge == NASR_MERGE_STACK_RESHAPE && D == 2;
    GemmDesc g{};
    g.A = ls->has_post ? ls->Ybuf[ls->npre].as<float>() : lc ? ls->lc_top.as<float>() : ls->outb[ls->L - 1].as<float>();
    g.B = h->P + ls->off_w;
    g.C = h->logits.as<float>();
    g.M = h->Tp * Bp; g.N = h->Cp; g.K = ls->Pinp;
    g.lda = sr ? Hp : ls->Pinp; g.ldb = h->Cp; g.ldc = h->Cp;
    g.a_map = sr ? h->rowmap_p : nullptr;
    g.a_rows = sr ? 2 * R : R;
    g.bias = h->P + ls->off_b;
    // N = Cp (32 for the 29 classes) gives the 128-row tiles of gemm.hip one block column: split K to fill the chip
    g.split_k = gemm_pick_split(g.M, g.N, g.K);
    if (int rc = gemm_f32(h, g)) return rc;
  }
  h->have_fwd = !chunk;
  return NASR_OK;
}

CtcDims ctc_dims(nasr_ctx* h) {
  CtcDims d;
  d.Tp = h->Tp; d.B = h->B; d.Bp = h->Bp; d.C = h->C; d.Cp = h->Cp; d.Lmax = std::max(h->Lmax, 1);
  d.KS = h->KS; d.Tws = h->T + 8;
  d.lprobs = h->ctcprobs.as<float>(); d.goff = h->ctckexp.as<double>();
  return d;
}

int ctc_forward(nasr_ctx* h) {
  PhaseScope ps(h, PH_PROJCTC);
  const CtcDims d = ctc_dims(h);
  launch_ctc_logz(d, h->logits.as<float>(), h->seq_p, h->logz.as<float>(), h->st);
  launch_ctc_alpha_beta(d, h->logits.as<float>(), h->logz.as<float>(), h->labels_p, h->lablen_p,
                        h->seq_p, h->alpha.as<float>(), h->beta.as<float>(), h->aoff.as<double>(),
                        h->boff.as<double>(), h->nll.as<float>(), h->logp.as<double>(), h->st);
  launch_mean(h->nll.as<float>(), h->B, h->loss.as<float>(), h->st);
  // the distillation term, while the student's logits are still logits: its gradient waits in kd_grad
  // for logit_grads, the loss becomes the combined one before anything publishes it
  h->kd_live = distill_on(h);
  if (h->kd_live) {
    const size_t rows = (size_t)h->Tp * h->Bp;
    bool grew = false;
    if (!h->kd_grad.ensure(rows * h->Cp * 4, &grew) || !h->kd_rows.ensure(rows * 4, &grew) ||
        !h->kd_sum.ensure((size_t)h->Bp * 8, &grew))
      return h->fail(NASR_ERR_HIP, "hipMalloc of the distillation term's buffers failed");
    launch_distill_rows(d, h->logits.as<float>(), h->teach.as<float>(), h->seq_p, h->kd_weight, h->kd_tau, h->kd_grad.as<float>(),
                        h->kd_rows.as<float>(), h->kd_sum.as<double>(), h->st);
    launch_distill_combine(h->kd_sum.as<double>(), h->B, h->kd_weight, h->kd_tau, h->loss.as<float>(), h->kd_parts.as<float>(),
                           h->kd_parts.as<float>() + 2, h->Gbase, h->st);
  }
  if (h->step_decode) {
    if (h->step_greedy)
      launch_greedy(d, h->logits.as<float>(), h->seq_p, h->amax.as<int>(), h->ids.as<int>(), h->lens.as<int>(), h->st);
    h->have_decoded = h->step_greedy;
    // what Network.train returns is known HERE, before the backward pass: copy it out now (nasr_get_step_results)
    h->res_cur ^= 1;
    nasr_ctx::StepRes& r = h->res[h->res_cur];
    const size_t ids_bytes = 8 + (size_t)h->Bp * 4 + (size_t)h->B * h->Tp * 4;
    const size_t lg_off = (ids_bytes + 255) / 256 * 256, lg_bytes = h->step_logits ? (size_t)h->Tp * h->Bp * h->Cp * 4 : 0;
    const size_t bytes = lg_off + lg_bytes;
    if (!pinned_ensure(r.host, &r.cap, bytes)) return h->fail(NASR_ERR_HIP, "hipHostMalloc of the step results failed");
    char* hp = static_cast<char*>(r.host.get());
    // the step's logits too (before the CTC gradient overwrites them in place): what tf.nn.ctc_beam_search_decoder reads in
    // the reference's train step (tfnetwork.py:61-64,188-189) - the host decodes them while the device runs on
    // They leave from a snapshot on a stream of their own: the compute stream pays a 1 MB device copy, not the PCIe transfer.
    if (lg_bytes) {
      bool grew = false;
      if (!h->logits_snap.ensure(lg_bytes, &grew)) return h->fail(NASR_ERR_HIP, "hipMalloc of the logits snapshot failed");
      if (!r.ev_lg) HIPCHK(h, hipEventCreateWithFlags(r.ev_lg.out(), hipEventDisableTiming));
      nasr_ctx::StepRes& prev = h->res[h->res_cur ^ 1];
      if (prev.logits && prev.ev_lg) HIPCHK(h, hipStreamWaitEvent(h->st, prev.ev_lg, 0));      // the snapshot's last reader (long done)
      HIPCHK(h, hipMemcpyAsync(h->logits_snap.p, h->logits.p, lg_bytes, hipMemcpyDeviceToDevice, h->st));
      HIPCHK(h, hipEventRecord(h->ev_snap, h->st));
      HIPCHK(h, hipStreamWaitEvent(h->d2h, h->ev_snap, 0));
      HIPCHK(h, hipMemcpyAsync(hp + lg_off, h->logits_snap.p, lg_bytes, hipMemcpyDeviceToHost, h->d2h));
      HIPCHK(h, hipEventRecord(r.ev_lg, h->d2h));
    }
    r.logits = lg_bytes != 0;
    r.seq = ++h->stamp_seq;
    // (enabled = 2: loss, fault word and logits only - the host runs its own decoder and has no use for the greedy one's)
    launch_publish_results(h->loss.as<float>(), h->Gbase, h->lens.as<int>(), h->step_greedy ? h->Bp : 0, h->ids.as<int>(),
                           h->step_greedy ? h->B * h->Tp : 0, r.host, r.stamp, r.seq, h->st);
    r.greedy = h->step_greedy;
    r.valid = true; r.B = h->B; r.Bp = h->Bp; r.Tp = h->Tp;
  }
  HIPCHK(h, hipGetLastError());
  return NASR_OK;
}

int loss_pass(nasr_ctx* h, bool training) {
  int rc;
  switch (h->family) {
    case Family::Las: return las_forward(h, true);   // the sequence loss is part of its forward pass
    case Family::WaveNet: rc = wn_forward(h, training); break;
    default: rc = forward(h); break;                 // clears the step's fault word
  }
  return rc ? rc : ctc_forward(h);
}

// weight / bias gradients of layer l from its complete dG, on stream ws: the main stream, or (side = true) the side stream
// with the 3-wave GEMM instantiation that shares the CUs with the persistent BPTT launch of the layer below
int weight_grads(nasr_ctx* h, int l, hipStream_t ws, bool side) {
  LstmState* const ls = h->lstm.get();
  const int Bp = h->Bp, D = ls->D, Hp = ls->Hp, N4 = ls->N4;
  const int R = ls->Tv * Bp;
  float* dG = dg_of(ls, l);
  unsigned char* GT = gttp_of(ls, l);
  float* cs_part = csws_of(ls, l);
  SV& gc = gc_of(ls, l);
  DevBuf& slab_buf = side ? ls->slabs2 : h->slabs;
  auto slabs_for = [&](int split, int M, int N) -> float* {
    if (split <= 1) return nullptr;
    bool grew = false;
    return slab_buf.ensure((size_t)split * M * N * 4, &grew) ? slab_buf.as<float>() : nullptr;
  };
  // a ragged batch contracts over its frames only (h->cmp_rows, nasr_ctx.h): every operand below is then gathered by vrow
  const int rows = h->cmp_rows ? h->cmp_rows : R;
  const int* vm = h->cmp_rows ? h->vrow_p : nullptr;
  const int nkb = (rows + 15) / 16;
  // The side instantiation splits K exactly as the main one would: every output element then sums the same k-blocks in
  // the same order whatever the tile shape - the gradients are bitwise those of the serial order.
  // one pass over dG: its transposed planes + 64-row partial column sums (already there when gemm_dx(l) ran)
  if (ls->gttp_layer != l) {
    dg_scales(h, l, R, false, ws);
    launch_tph_split2(dG, nullptr, GT, rows, D * N4, D * N4, nullptr, 1.f, gc.sp(), 1.f, cs_part, ws, vm);
  }
  ls->gttp_layer = -1;
  const ActScale ao = act_out(ls), ai = lstm_in_scale(ls, l);
  // out[l-1] (input weight gradient) and out[l] (recurrent weight gradient) with the frame index as contraction index, where
  // the forward pass has not left them (gemm_xproj).  Compacted rows: out[l] is wanted SHIFTED by one frame, which is no
  // constant row offset there - its planes are built here from the rows vprev (forward direction's columns) / vnext
  // (backward direction's), and the plain transposed planes of out[l] are not needed at all.
  for (int m = std::max(l - 1, 0); m <= (vm ? l - 1 : l); ++m)
    if (!ls->ott_valid[m]) {
      launch_tph_split2(ls->outb[m].as<float>(), nullptr, ls->OTT[m].as<unsigned char>(), rows, D * Hp, D * Hp, nullptr, 1.f, ao.cs, 1.f,
                        nullptr, ws, vm);
      ls->ott_valid[m] = 1;
    }
  unsigned char* OS = ls->OTS.as<unsigned char>() + (wg_alt(ls, l) ? tph_bytes(D * Hp, R) : 0);
  if (vm)
    launch_tph_split2(ls->outb[l].as<float>(), nullptr, OS, rows, D * Hp, D * Hp, nullptr, 1.f, ao.cs, 1.f, nullptr, ws, h->vprev_p,
                      D == 2 ? h->vnext_p : nullptr, Hp);
  if (l == 0 && ls->npre)
    pl_split(lstm_input(h, l), nullptr, ls->X0TTP.as<unsigned char>(), R, ls->Ip[0], ls->Ip[0], nullptr, ai.cs, nullptr, ws);
  {  // dWx = X^T dG
    GemmTPHDesc g{};
    g.A = l == 0 ? ls->X0TTP.as<unsigned char>() : ls->OTT[l - 1].as<unsigned char>();
    g.B = GT; g.C = h->G + ls->off_wx[l];
    g.M = ls->Ip[l]; g.N = D * N4; g.K = rows; g.nkbA = nkb; g.nkbB = nkb; g.ldc = D * N4;
    g.side = side;
    g.split_k = gemm_tph_pick_split(g.M, g.N, g.K);
    g.slabs = slabs_for(g.split_k, g.M, g.N);
    if (g.split_k > 1 && !g.slabs) return h->fail(NASR_ERR_HIP, "slab workspace allocation failed");
    pl_gemm(g, ai.cinv, gc.ip(), ws);
  }
  launch_colsum_parts(cs_part, tp_split2_parts(rows), D * N4, h->G + ls->off_bias[l], ws);
  {  // dU = shift(H)^T dG : h_prev of frame t is out[t-1] (fw) / out[t+1] (bw); both directions in one launch
    GemmTPHDesc g{};
    g.A = vm ? OS : ls->OTT[l].as<unsigned char>(); g.B = GT; g.C = h->G + ls->off_u[(size_t)l * D];
    g.M = Hp; g.N = N4; g.K = rows; g.nkbA = nkb; g.nkbB = nkb; g.ldc = N4;
    g.a_kshift = vm ? 0 : -Bp;
    g.nbatch = D;
    g.a_bstride = (size_t)(Hp / 32) * pl_rb_bytes(nkb); g.b_bstride = (size_t)(N4 / 32) * pl_rb_bytes(nkb);
    g.c_bstride = (int64_t)Hp * N4;            // off_u[l*D + 1] - off_u[l*D] (build_layout)
    g.a_kshift1 = vm ? 0 : Bp;
    g.side = side;
    g.split_k = gemm_tph_pick_split(g.M, g.N, g.K, D);
    g.slabs = slabs_for(g.split_k * D, g.M, g.N);
    if (g.split_k > 1 && !g.slabs) return h->fail(NASR_ERR_HIP, "slab workspace allocation failed");
    pl_gemm(g, ao.cinv, gc.ip(), ws, Hp, N4);
  }
  HIPCHK(h, hipGetLastError());
  return NASR_OK;
}

// the main stream waits for layer l's side-stream weight gradients (no-op when there are none outstanding)
int wg_join(nasr_ctx* h, int l) {
  LstmState* const ls = h->lstm.get();
  if (l >= 0 && l < ls->L && ls->wg_pending[l]) {
    HIPCHK(h, hipStreamWaitEvent(h->st, ls->ev_wg[l], 0));
    ls->wg_pending[l] = 0;
  }
  return NASR_OK;
}

int backward(nasr_ctx* h) {
  switch (h->family) {
    case Family::WaveNet: return wn_backward(h);
    case Family::Las: return las_backward(h);
    default: return lstm_backward(h);
  }
}

int logit_grads(nasr_ctx* h) {
  PhaseScope ps(h, PH_PROJCTC);
  const CtcDims d = ctc_dims(h);
  const float scale = h->kd_live ? (1.f - h->kd_weight) / (float)h->B : 1.f / (float)h->B;
  launch_ctc_grad(d, h->logits.as<float>(), h->logz.as<float>(), h->lablen_p, h->seq_p, h->cstart_p, h->cpos_p,
                  h->alpha.as<float>(), h->beta.as<float>(), h->aoff.as<double>(), h->boff.as<double>(), h->logp.as<double>(),
                  scale, h->st);
  if (h->kd_live) launch_distill_add(d, h->logits.as<float>(), h->kd_grad.as<float>(), h->st);
  HIPCHK(h, hipGetLastError());
  h->have_fwd = false;   // the logits are gone (nasr_take_teacher_logits asks)
  return NASR_OK;
}

int lstm_backward(nasr_ctx* h) {
  LstmState* const ls = h->lstm.get();
  const int Bp = h->Bp, T = h->T, D = ls->D, Hp = ls->Hp;
  const int R = T * Bp, Rp = h->Tp * Bp, Rv = ls->Tv * Bp;
  const bool sr = ls->cfg.merge == NASR_MERGE_STACK_RESHAPE && D == 2;
  const bool lc = ls->lc_live;
  const RecKind use = lc ? RecKind::Step : ls->rec_use;   // a chunked batch: the per-step kernels, whatever the handle's kind
  if (use == RecKind::Persist) {
    HIPCHK(h, hipMemsetAsync(ls->pctl + 1 + ls->L, 0, (size_t)ls->L * sizeof(PersistCtl), h->st));
    HIPCHK(h, hipMemsetAsync(ls->xchb, 0, (size_t)ls->L * persist_px_bytes(), h->st));   // epoch 0 everywhere (lstm_persist.hip)
  }
  if (int rc = logit_grads(h)) return rc;
  {
    PhaseScope ps(h, PH_PROJB);
    // dW = gather(out)^T dlogits
    GemmDesc g{};
    g.A = ls->has_post ? ls->Ybuf[ls->npre].as<float>() : lc ? ls->lc_top.as<float>() : ls->outb[ls->L - 1].as<float>();
    g.B = h->logits.as<float>();
    g.C = h->G + ls->off_w;
    g.M = ls->Pinp; g.N = h->Cp; g.K = Rp;
    g.lda = sr ? Hp : ls->Pinp; g.ldb = h->Cp; g.ldc = h->Cp;
    g.a_col = true; g.a_map = sr ? h->rowmap_p : nullptr; g.a_rows = sr ? 2 * R : R;
    g.split_k = gemm_pick_split(g.M, g.N, g.K);
    if (int rc = gemm_f32(h, g)) return rc;
    launch_colsum(h->logits.as<float>(), Rp, h->Cp, h->Cp, h->G + ls->off_b, ls->csws.as<float>(), h->st);
    // dOut_last = scatter(dlogits W^T)
    GemmDesc x{};
    x.A = h->logits.as<float>();
    x.B = h->P + ls->off_w;
    x.C = ls->has_post ? ls->dYbuf[ls->npre].as<float>() : lc ? ls->lc_dtop.as<float>() : dout_of(ls, ls->L - 1);
    x.M = Rp; x.N = ls->Pinp; x.K = h->Cp;
    x.lda = h->Cp; x.ldb = h->Cp; x.ldc = sr ? Hp : ls->Pinp;
    x.b_col = true; x.a_rows = Rp; x.c_map = sr ? h->rowmap_p : nullptr; x.split_k = 1;
    if (int rc = gemm_f32(h, x)) return rc;
    // ... back onto the windows' rows: the look-ahead rows get no gradient from above
    if (lc) launch_lc_scatter(ls->lc_dtop.as<float>(), h->seq_p, h->wlen_p, dout_of(ls, ls->L - 1), ls->lcg, D * Hp, h->st);
  }
  if (ls->has_post) {
    PhaseScope ps(h, PH_WGRAD);
    int rc = dense_backward(h, ls->npre, ls->outb[ls->L - 1].as<float>(), dout_of(ls, ls->L - 1));
    if (rc) return rc;
  }
  h->n_bwd_launch = 0;
  ls->dgmax_layer = -1;
  for (int l = ls->L - 1; l >= 0; --l) {
    const bool defer = use != RecKind::Step && ls->bucket_defer;
    {
      PhaseScope ps(h, PH_RECB);
      int rc = lc ? lc_run_steps(h, l, true, h->st, &h->n_bwd_launch) : run_steps(h, l, true, h->st, &h->n_bwd_launch);
      if (rc) return rc;
    }
    if (defer && l + 1 < ls->L && ls->bucket_of_layer[l + 1] >= 0) {   // the layer above's bucket, held back over this launch
      if (int rc = wg_join(h, l + 1)) return rc;
      HIPCHK(h, hipEventRecord(h->ev_bucket[ls->bucket_of_layer[l + 1]], h->st));
    }
    PhaseScope ps(h, PH_WGRAD);
    // layer l+2's side-stream weight gradients read the plane buffers this layer's passes are about to rewrite (they
    // finished a BPTT launch ago: the wait costs nothing, it only makes the order formal)
    if (int rc = wg_join(h, l + 2)) return rc;
    if (l > 0 || ls->npre > 0) gemm_dx(h, l, Rv, h->st);   // critical path first
    // layer l's weight gradients feed nothing before Adam: with the overlap on they leave the main stream here and run
    // beside the persistent BPTT launch of layer l-1 (tfnetwork.py:120-128: the gradients are a set, nothing orders them)
    const bool side = ls->wg_overlap && use == RecKind::Persist && l > 0 && ls->gttp_layer == l;
    if (side) {
      HIPCHK(h, hipEventRecord(ls->ev_dx, h->st));
      HIPCHK(h, hipStreamWaitEvent(ls->wst, ls->ev_dx, 0));
      int rc = weight_grads(h, l, ls->wst, true);
      if (rc) return rc;
      HIPCHK(h, hipEventRecord(ls->ev_wg[l], ls->wst));
      ls->wg_pending[l] = 1;
    } else {
      int rc = weight_grads(h, l, h->st, false);
      if (rc) return rc;
    }
    if (ls->bucket_of_layer[l] >= 0 && !(defer && l > 0)) {
      if (int rc = wg_join(h, l)) return rc;
      HIPCHK(h, hipEventRecord(h->ev_bucket[ls->bucket_of_layer[l]], h->st));
    }
  }
  for (int l = 0; l < ls->L; ++l)
    if (int rc = wg_join(h, l)) return rc;     // whatever is still out: before the last bucket / Adam
  for (int i = ls->npre - 1; i >= 0; --i) {
    PhaseScope ps(h, PH_WGRAD);
    int rc = dense_backward(h, i, i == 0 ? h->X0.as<float>() : ls->Ybuf[i - 1].as<float>(),
                            i > 0 ? ls->dYbuf[i - 1].as<float>() : nullptr);
    if (rc) return rc;
  }
  HIPCHK(h, hipEventRecord(h->ev_bucket.back(), h->st));   // the bucket with the fault word: nothing of the step is left
  h->have_grads = true;
  return NASR_OK;
}

int fetch_logits(nasr_ctx* h, float* logits_out, int rows) {
  const int Tr = rows >= 0 ? std::min(rows, h->Tp) : h->Tp;
  const size_t n = (size_t)Tr * h->Bp * h->Cp;
  std::vector<float> host(n);
  HIPCHK(h, hipMemcpyAsync(host.data(), h->logits.p, n * 4, hipMemcpyDeviceToHost, h->st));
  if (int rc = sync_checked(h)) return rc;
  for (int t = 0; t < Tr; ++t)
    for (int b = 0; b < h->B; ++b)
      memcpy(logits_out + ((size_t)t * h->B + b) * h->C, host.data() + ((size_t)t * h->Bp + b) * h->Cp,
             (size_t)h->C * 4);
  return NASR_OK;
}

}  // namespace nasr_impl
