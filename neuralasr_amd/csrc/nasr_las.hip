// nasr_las.hip — the LAS network of the reference (networks/las.py: Listen, Attend and Spell): a 4-layer pyramidal BiLSTM
// encoder (250 units per direction, odd lengths padded by one zero frame, frame pairs concatenated between layers, both
// directions over every padded frame) and an attention decoder (BasicLSTMCell(500) in an AttentionWrapper with
// unnormalised Bahdanau attention over the top layer's output, attention layer 250, projection to the classes), trained
// with scheduled sampling and sequence_loss.  This file holds the handle's create call, parameter layout, buffers and the
// forward / backward pass, and the beam search; the kernels are in las.hip, las_beam.hip and gemm.hip.  The
// training pass and the search run the same encoder loop (las_encode, each over a LasEnc of its own) and the same decoder
// step (las_decoder_step).  Opening and finishing the handle, batches, Adam, gradient exchange and checkpoints are the
// common code.  DESIGN.md §10.
#include "nasr_ctx.h"
#include "las.h"
#include "las_beam.h"

#include <functional>

using namespace nasr;
using namespace nasr_impl;

namespace nasr_impl {

// One set of encoder activations, rows Lr[l] * Bp per layer: the training pass has one, the beam search another
struct LasEnc {
  static constexpr int NL = 4;
  int Lr[NL] = {0, 0, 0, 0};   // frames each layer runs over: L1 = T + T%2, L(i+1) = L(i)/2 + (L(i)/2)%2
  DevBuf X[NL], xp[NL], act[NL], c[NL], out[NL];
  // sizes the buffers for T frames of Bp rows and sets Lr; false: an allocation failed
  bool ensure(int T, int Bp, bool* grew) {
    bool ok = true;
    for (int l = 0, L = T + T % 2; l < NL; ++l, L = L / 2 + (L / 2) % 2) {
      const size_t R = (size_t)L * Bp;
      Lr[l] = L;
      if (l > 0) ok &= X[l].ensure(R * 4 * LAS_HE * 4, grew);
      ok &= xp[l].ensure(R * 2 * LAS_G4E * 4, grew);
      ok &= act[l].ensure(R * 2 * LAS_G4E * 4, grew);
      ok &= c[l].ensure(R * 2 * LAS_H * 4, grew);
      ok &= out[l].ensure(R * 2 * LAS_HE * 4, grew);
    }
    return ok;
  }
};

// The beam search's own buffers (nasr_las_beam_search), made on the first search and apart from the training pass's: a
// search leaves the resident batch, the last pass's logits and loss, the gradient and the sampling state as they are.
// Beam rows r = b*W + k, R = rup(B*W, 16); the encoder's rows t*Bp + b as in training.
struct LasBeam {
  int B = 0, Bp = 0, T = 0, W = 0, R = 0, max_steps = 0, Tdec = 0, end_id = 0;
  bool have = false, timed = false;
  LasEnc enc;
  DevBuf feats, X0, keys;
  // decoder rows: S / c the beams' state, Sx / cx the step's outputs before the gather by parent
  DevBuf S, cs, Sx, cx, gp, dact, HC, Q, logits, ids;
  DevBuf logp[2], len[2], fin[2], ctx[2];          // ping-pong by step parity: step t reads [t & 1], writes the other
  DevBuf scores, totals, sel_idx, sel_score, pen, flags;
  DevBuf tr_score, tr_word, tr_parent, gathered;   // [max_steps][B*W]
  std::vector<float> hpen;
  std::vector<Event> ev;                           // phase marks of a timed search
  std::vector<std::pair<int, size_t>> marks;
  float times[7] = {0, 0, 0, 0, 0, 0, 0};
};

struct LasState {
  nasr_las_cfg cfg;
  // internal parameter layout (floats from P): per layer Wx [Ip][2*G4E] (fw | bw gate columns), Wh fw / bw [LAS_HE][G4E],
  // bias [2*G4E]; memory_layer [512][512]; the decoder kernel's one-hot rows E [C][G4D], its [a; h] rows Wah [768][G4D],
  // its bias; query_layer [512][512]; attention_v [512]; attention_layer [1024][256]; projection [256][Cp], bias [Cp]
  int Ip[LasEnc::NL];
  int64_t off_wx[LasEnc::NL], off_whf[LasEnc::NL], off_whb[LasEnc::NL], off_b[LasEnc::NL];
  int64_t off_wmem = 0, off_e = 0, off_wah = 0, off_bd = 0, off_wq = 0, off_v = 0, off_watt = 0, off_wp = 0, off_bp = 0;
  // scheduled sampling: probability, hash seed, pass counter, tower (las.hip)
  float p = 0.1f;
  uint32_t seed = 1u, counter = 0u;
  int tower = 0;
  // shape of the resident batch and its encoder activations
  int U = 0;
  bool have_pass = false;
  LasEnc enc;
  DevBuf dGe, dX, dout, dhc, dcc, whT;   // whT: [2][G4E][LAS_HE] the layer's recurrent matrices transposed (BPTT)
  // attention and decoder
  DevBuf keys, dkeys, dmem, tmpm;
  DevBuf S, cinit, dc, dact, gp, Q, alpha, HC, logits, ids, sampled;
  DevBuf dL, wce, w, tmpA, dA, dHC, dQ, dhq, dGd, dS, dcd, dvpart, csws;
  std::unique_ptr<LasBeam> beam;   // the beam search's buffers (first search)
  // n-gram fusion of the search (nasr_las_beam_set_lm): the dense table [lm_K][C] on the device, lm_K = C^(order-1)
  DevBuf lm;
  int lm_order = 0, lm_K = 1;
  float lm_weight = 0.f;
};

int las_layout(nasr_ctx* h) {
  LasState& s = *h->las;
  const int C = s.cfg.num_classes;
  h->F = s.cfg.feature_size;
  h->C = C;
  h->Fp = rup(h->F, 32);
  h->Cp = rup(C, 32);
  int64_t off = 0;
  for (int l = 0; l < LasEnc::NL; ++l) {
    s.Ip[l] = l == 0 ? h->Fp : 4 * LAS_HE;
    s.off_wx[l] = off; off += (int64_t)s.Ip[l] * 2 * LAS_G4E;
    s.off_whf[l] = off; off += (int64_t)LAS_HE * LAS_G4E;
    s.off_whb[l] = off; off += (int64_t)LAS_HE * LAS_G4E;
    s.off_b[l] = off; off += 2 * LAS_G4E;
  }
  s.off_wmem = off; off += (int64_t)LAS_HD * LAS_HD;
  s.off_e = off; off += (int64_t)C * LAS_G4D;
  s.off_wah = off; off += (int64_t)LAS_SW * LAS_G4D;
  s.off_bd = off; off += LAS_G4D;
  s.off_wq = off; off += (int64_t)LAS_HD * LAS_HD;
  s.off_v = off; off += LAS_HD;
  s.off_watt = off; off += (int64_t)2 * LAS_HD * LAS_HE;
  s.off_wp = off; off += (int64_t)LAS_HE * h->Cp;
  s.off_bp = off; off += h->Cp;
  h->np_int = off;

  h->tensors.clear();
  h->tf2int.clear();
  int64_t tf = 0;
  // rows x cols in TF order; where(r, c) = the internal index of element (r, c)
  auto add = [&](const std::string& name, int64_t rows, int64_t cols, const std::function<int64_t(int64_t, int64_t)>& where) {
    h->tensors.push_back({name, tf, rows, cols});
    for (int64_t r = 0; r < rows; ++r)
      for (int64_t c = 0; c < cols; ++c) h->tf2int.push_back((int32_t)where(r, c));
    tf += rows * cols;
  };
  for (int l = 0; l < LasEnc::NL; ++l) {
    const int I = l == 0 ? h->F : 4 * LAS_H;
    auto in_row = [l](int64_t r) -> int64_t {   // TF input row -> internal row of Wx (layers >= 1: the pair layout)
      if (l == 0) return r;
      const int64_t p = r / (2 * LAS_H), q = r % (2 * LAS_H);
      return p * 2 * LAS_HE + las_memcol((int)q);
    };
    for (int d = 0; d < 2; ++d) {
      const std::string dn = d == 0 ? "fw" : "bw";
      const std::string scope = "bidirectional_rnn/" + dn + "/" + dn + "_" + std::to_string(l);
      const int64_t whoff = d == 0 ? s.off_whf[l] : s.off_whb[l];
      add(scope + "/kernel", I + LAS_H, LAS_G4E, [&](int64_t r, int64_t c) {
        return r < I ? s.off_wx[l] + in_row(r) * 2 * LAS_G4E + d * LAS_G4E + c : whoff + (r - I) * LAS_G4E + c;
      });
      add(scope + "/bias", LAS_G4E, 1, [&](int64_t r, int64_t) { return s.off_b[l] + d * LAS_G4E + r; });
    }
  }
  add("memory_layer/kernel", 2 * LAS_H, 2 * LAS_H,
      [&](int64_t r, int64_t c) { return s.off_wmem + (int64_t)las_memcol((int)r) * LAS_HD + c; });
  add("decoder_lstm/kernel", C + LAS_H + 2 * LAS_H, LAS_G4D, [&](int64_t r, int64_t c) {
    if (r < C) return s.off_e + r * LAS_G4D + c;
    if (r < C + LAS_H) return s.off_wah + (r - C) * LAS_G4D + c;
    return s.off_wah + (LAS_HE + r - C - LAS_H) * LAS_G4D + c;
  });
  add("decoder_lstm/bias", LAS_G4D, 1, [&](int64_t r, int64_t) { return s.off_bd + r; });
  add("query_layer/kernel", 2 * LAS_H, 2 * LAS_H, [&](int64_t r, int64_t c) { return s.off_wq + r * LAS_HD + c; });
  add("attention_v", 2 * LAS_H, 1, [&](int64_t r, int64_t) { return s.off_v + r; });
  add("attention_layer/kernel", 4 * LAS_H, LAS_H, [&](int64_t r, int64_t c) {
    const int64_t row = r < 2 * LAS_H ? r : LAS_HD + las_memcol((int)(r - 2 * LAS_H));
    return s.off_watt + row * LAS_HE + c;
  });
  add("projection_layer/kernel", LAS_H, C, [&](int64_t r, int64_t c) { return s.off_wp + r * h->Cp + c; });
  add("projection_layer/bias", C, 1, [&](int64_t r, int64_t) { return s.off_bp + r; });
  h->np_tf = tf;
  return NASR_OK;
}

int las_ensure_shape(nasr_ctx* h, int B, int T, int Lmax) {
  LasState& s = *h->las;
  const int Bp = rup(B, 16);
  bool grew = false, ok = s.enc.ensure(T, Bp, &grew);
  const int U = std::max(Lmax, 1), L4 = s.enc.Lr[LasEnc::NL - 1];
  const size_t R0 = (size_t)s.enc.Lr[0] * Bp, UB = (size_t)U * Bp, MB = (size_t)L4 * Bp;
  ok &= h->X0.ensure((size_t)T * Bp * h->Fp * 4, &grew);
  ok &= h->seqbuf.ensure((size_t)Bp * 4, &grew);
  ok &= h->loss.ensure(16, &grew);
  ok &= h->nll.ensure((size_t)Bp * 4, &grew);
  ok &= s.dGe.ensure(R0 * 2 * LAS_G4E * 4, &grew);
  ok &= s.dX.ensure(R0 * 4 * LAS_HE * 4, &grew);
  ok &= s.dout.ensure(R0 * 2 * LAS_HE * 4, &grew);
  ok &= s.whT.ensure((size_t)2 * LAS_G4E * LAS_HE * 4, &grew);
  ok &= s.dhc.ensure((size_t)2 * Bp * LAS_HE * 4, &grew) && s.dcc.ensure((size_t)2 * Bp * LAS_HE * 4, &grew);
  for (DevBuf* m : {&s.keys, &s.dkeys, &s.dmem, &s.tmpm}) ok &= m->ensure(MB * LAS_HD * 4, &grew);
  ok &= s.S.ensure((UB + Bp) * LAS_SW * 4, &grew);
  ok &= s.cinit.ensure((size_t)Bp * LAS_HD * 4, &grew);
  ok &= s.dc.ensure(UB * LAS_HD * 4, &grew);
  ok &= s.dact.ensure(UB * LAS_G4D * 4, &grew);
  ok &= s.gp.ensure((size_t)Bp * LAS_G4D * 4, &grew);
  ok &= s.Q.ensure(UB * LAS_HD * 4, &grew);
  ok &= s.alpha.ensure(UB * L4 * 4, &grew);
  ok &= s.HC.ensure(UB * 2 * LAS_HD * 4, &grew);
  ok &= s.logits.ensure(UB * h->Cp * 4, &grew);
  ok &= s.ids.ensure(UB * 4, &grew) && s.sampled.ensure(UB * 4, &grew);
  ok &= s.dL.ensure(UB * h->Cp * 4, &grew);
  ok &= s.wce.ensure(UB * 4, &grew) && s.w.ensure(UB * 4, &grew);
  ok &= s.tmpA.ensure((size_t)Bp * LAS_HE * 4, &grew);
  ok &= s.dA.ensure(UB * LAS_HE * 4, &grew);
  ok &= s.dHC.ensure((size_t)Bp * 2 * LAS_HD * 4, &grew);
  ok &= s.dQ.ensure(UB * LAS_HD * 4, &grew);
  ok &= s.dhq.ensure((size_t)Bp * LAS_HD * 4, &grew);
  ok &= s.dGd.ensure(UB * LAS_G4D * 4, &grew);
  ok &= s.dS.ensure((size_t)Bp * LAS_SW * 4, &grew);
  ok &= s.dcd.ensure((size_t)Bp * LAS_HD * 4, &grew);
  ok &= s.dvpart.ensure(UB * LAS_HD * 4, &grew);
  // launch_colsum's 32 partial rows of the widest matrix the backward pass sums: dGe, dGd or dL (Cp has no upper bound)
  ok &= s.csws.ensure((size_t)32 * std::max({2 * LAS_G4E, LAS_G4D, h->Cp}) * 4, &grew);
  if (!ok) return h->fail(NASR_ERR_HIP, "hipMalloc failed while sizing batch buffers");
  h->B = B; h->Bp = Bp; h->T = T; h->Lmax = Lmax; h->Tp = U; h->KS = 1;
  s.U = U;
  return NASR_OK;
}

// The pyramidal encoder over X0 [T*Bp][Fp] (rows t*Bp + b, Bp = rup(B, 16)) into e, sized by e.ensure(T, Bp).  The
// training pass and the beam search share it.
int las_encode(nasr_ctx* h, const float* X0, int T, int B, LasEnc& e) {
  LasState& s = *h->las;
  const int Bp = rup(B, 16);
  const float* P = h->P;
  hipStream_t st = h->st;
  for (int l = 0; l < LasEnc::NL; ++l) {
    const int L = e.Lr[l];
    const float* Xin = l == 0 ? X0 : fp(e.X[l]);
    // rows past the input's frames (the odd-length padding) read as zero
    const int in_rows = (l == 0 ? T : e.Lr[l - 1] / 2) * Bp;
    if (l > 0) launch_las_pyr_pack(fp(e.out[l - 1]), fp(e.X[l]), e.Lr[l - 1] / 2, Bp, st);
    if (int rc = gemm_dense(h, Xin, P + s.off_wx[l], fp(e.xp[l]), L * Bp, 2 * LAS_G4E, s.Ip[l], s.Ip[l], 2 * LAS_G4E,
                            2 * LAS_G4E, false, false, P + s.off_b[l], 0, in_rows))
      return rc;
    for (int t = 0; t < L; ++t)
      launch_las_enc_fwd_step(fp(e.xp[l]), P + s.off_whf[l], P + s.off_whb[l], fp(e.act[l]), fp(e.c[l]), fp(e.out[l]), t, L, B,
                              Bp, st);
  }
  return NASR_OK;
}

// phases of a timed beam search (nasr_las_beam_get_times)
enum { LB_ENC = 0, LB_GEMM, LB_CELL, LB_ATTN, LB_SEL, LB_TREE, LB_WAIT, LB_COUNT };

// One decoder step over `rows` decoder rows (the training pass's utterances, the search's beams).
struct LasStep {
  const float* S;         // the step's input rows [a | h] [rows][LAS_SW]
  const int32_t* ids;     // the ids fed to the step
  const float* cprev;     // the cell state before it
  float *gp, *act, *c;    // the gate product (scratch), the gate activations and the cell state after it
  float* Snext;           // [a | h] of the next step
  float *HC, *Q, *logits;
  // attention: the keys and the memory [L4*Bp][LAS_HD], W rows per utterance, rows >= nrows padding, alpha [rows][L4] or
  // nullptr, the search's done word or nullptr
  const float *keys, *mem;
  int L4, Bp, W, nrows;
  float* alpha;
  const int32_t* done;
};

// Enqueues the step: gate GEMM on [a | h] W_ah, the cell, the query GEMM, attention, the attention-layer and projection
// GEMMs.  mark (may be empty): called with the phase just enqueued (LB_GEMM, LB_CELL, LB_GEMM, LB_ATTN, LB_GEMM).
int las_decoder_step(nasr_ctx* h, int rows, const LasStep& k, const std::function<void(int)>& mark) {
  const LasState& s = *h->las;
  const float* P = h->P;
  const int Cp = h->Cp;
  hipStream_t st = h->st;
  if (int rc = gemm_dense(h, k.S, P + s.off_wah, k.gp, rows, LAS_G4D, LAS_SW, LAS_SW, LAS_G4D, LAS_G4D, false, false)) return rc;
  if (mark) mark(LB_GEMM);
  launch_las_dec_cell(k.gp, P + s.off_e, P + s.off_bd, k.ids, k.cprev, k.act, k.c, k.Snext, k.HC, rows, st);
  if (mark) mark(LB_CELL);
  if (int rc = gemm_dense(h, k.Snext + LAS_HE, P + s.off_wq, k.Q, rows, LAS_HD, LAS_HD, LAS_SW, LAS_HD, LAS_HD, false, false))
    return rc;
  if (mark) mark(LB_GEMM);
  launch_las_attend(k.keys, k.mem, k.Q, P + s.off_v, k.alpha, k.HC, k.L4, k.Bp, k.W, k.nrows, rows, k.done, st);
  if (mark) mark(LB_ATTN);
  if (int rc = gemm_dense(h, k.HC, P + s.off_watt, k.Snext, rows, LAS_HE, 2 * LAS_HD, 2 * LAS_HD, LAS_HE, LAS_SW, false, false))
    return rc;
  if (int rc = gemm_dense(h, k.Snext, P + s.off_wp, k.logits, rows, Cp, LAS_HE, LAS_SW, Cp, Cp, false, false, P + s.off_bp))
    return rc;
  if (mark) mark(LB_GEMM);
  return NASR_OK;
}

// The encoder and the decoder chain of the resident batch.  sample: scheduled sampling with the handle's probability (one
// counter value per such pass); otherwise every step is fed its label.
int las_forward(nasr_ctx* h, bool sample) {
  if (!h->resident) return h->fail(NASR_ERR_STATE, "no resident batch: call nasr_upload_batch first");
  if (h->Lmax < 1) return h->fail(NASR_ERR_ARG, "the LAS decoder needs labels (U = labels.shape[1] >= 1)");
  LasState& s = *h->las;
  const int B = h->B, Bp = h->Bp, U = s.U, C = h->C, Cp = h->Cp;
  const float* P = h->P;
  hipStream_t st = h->st;
  HIPCHK(h, hipMemsetAsync(h->Gbase, 0, GRAD_HEAD * 4, st));   // the step's fault word (nothing here raises it)
  {
    PhaseScope ps(h, PH_RECF);
    if (int rc = las_encode(h, h->X0.as<float>(), h->T, B, s.enc)) return rc;
  }
  PhaseScope ps(h, PH_PROJCTC);
  const int L4 = s.enc.Lr[LasEnc::NL - 1];
  const float* mem = fp(s.enc.out[LasEnc::NL - 1]);
  if (int rc = gemm_dense(h, mem, P + s.off_wmem, fp(s.keys), L4 * Bp, LAS_HD, LAS_HD, LAS_HD, LAS_HD, LAS_HD, false, false))
    return rc;
  launch_las_dec_init(mem, fp(s.enc.c[LasEnc::NL - 1]), h->labels_p, h->Lmax, L4, B, Bp, fp(s.S), fp(s.cinit), s.ids.as<int32_t>(),
                      st);
  LasSample smp{};
  if (sample && s.p > 0.f) {
    smp.on = 1;
    smp.p = s.p;
    smp.thr = s.p >= 1.f ? (1u << 24) : (uint32_t)std::floor((double)s.p * 16777216.0);
    smp.key = s.seed + 0x9E3779B9u * (uint32_t)(s.tower + 1) + 0x85EBCA6Bu * s.counter;
  }
  if (sample) s.counter += 1;
  HIPCHK(h, hipMemsetAsync(s.sampled.p, 0, (size_t)Bp * 4, st));
  for (int t = 0; t < U; ++t) {
    float* St = fp(s.S, (size_t)t * Bp * LAS_SW);
    float* lg = fp(s.logits, (size_t)t * Bp * Cp);
    LasStep k{};
    k.S = St; k.ids = s.ids.as<int32_t>() + (size_t)t * Bp;
    k.cprev = t == 0 ? fp(s.cinit) : fp(s.dc, (size_t)(t - 1) * Bp * LAS_HD);
    k.gp = fp(s.gp); k.act = fp(s.dact, (size_t)t * Bp * LAS_G4D); k.c = fp(s.dc, (size_t)t * Bp * LAS_HD);
    k.Snext = St + (size_t)Bp * LAS_SW;
    k.HC = fp(s.HC, (size_t)t * Bp * 2 * LAS_HD); k.Q = fp(s.Q, (size_t)t * Bp * LAS_HD); k.logits = lg;
    k.keys = fp(s.keys); k.mem = mem; k.L4 = L4; k.Bp = Bp;
    k.W = 1; k.nrows = Bp;   // every row, the padded ones too, runs the attention body
    k.alpha = fp(s.alpha, (size_t)t * Bp * L4);
    if (int rc = las_decoder_step(h, Bp, k, nullptr)) return rc;
    if (t + 1 < U)
      launch_las_sample(lg, Cp, C, h->labels_p, h->Lmax, t, B, Bp, smp, s.ids.as<int32_t>() + (size_t)(t + 1) * Bp,
                        s.sampled.as<int32_t>() + (size_t)(t + 1) * Bp, st);
  }
  launch_las_ce(fp(s.logits), h->labels_p, h->lablen_p, h->Lmax, U, B, Bp, C, Cp, fp(s.dL), fp(s.wce), fp(s.w), st);
  launch_las_loss(fp(s.wce), fp(s.w), U, B, Bp, h->loss.as<float>(), h->nll.as<float>(), fp(s.dL), Cp, st);
  HIPCHK(h, hipGetLastError());
  s.have_pass = true;
  h->have_fwd = true;
  return NASR_OK;
}

int las_backward(nasr_ctx* h) {
  LasState& s = *h->las;
  const int B = h->B, Bp = h->Bp, U = s.U, C = h->C, Cp = h->Cp;
  const int L4 = s.enc.Lr[LasEnc::NL - 1];
  const int UB = U * Bp;
  const float* P = h->P;
  float* G = h->G;
  hipStream_t st = h->st;
  const float* mem = fp(s.enc.out[LasEnc::NL - 1]);
  {
    PhaseScope ps(h, PH_PROJB);
    for (int t = U - 1; t >= 0; --t) {
      const bool last = t == U - 1;
      const float* dLt = fp(s.dL, (size_t)t * Bp * Cp);
      float* dAt = fp(s.dA, (size_t)t * Bp * LAS_HE);
      float* dQt = fp(s.dQ, (size_t)t * Bp * LAS_HD);
      // da_t = dlogits W_p^T (+ the next step's gate input)
      if (int rc = gemm_dense(h, dLt, P + s.off_wp, last ? dAt : fp(s.tmpA), Bp, LAS_HE, Cp, Cp, Cp, LAS_HE, false, true)) return rc;
      if (!last) launch_las_add(fp(s.tmpA), LAS_HE, fp(s.dS), LAS_SW, dAt, LAS_HE, Bp, LAS_HE, st);
      if (int rc = gemm_dense(h, dAt, P + s.off_watt, fp(s.dHC), Bp, 2 * LAS_HD, LAS_HE, LAS_HE, LAS_HE, 2 * LAS_HD, false, true))
        return rc;
      launch_las_attend_bwd(fp(s.keys), mem, fp(s.Q, (size_t)t * Bp * LAS_HD), P + s.off_v, fp(s.alpha, (size_t)t * Bp * L4),
                            fp(s.dHC), dQt, fp(s.dkeys), fp(s.dmem), fp(s.dvpart, (size_t)t * Bp * LAS_HD), L4, Bp, last, st);
      if (int rc = gemm_dense(h, dQt, P + s.off_wq, fp(s.dhq), Bp, LAS_HD, LAS_HD, LAS_HD, LAS_HD, LAS_HD, false, true)) return rc;
      float* dGt = fp(s.dGd, (size_t)t * Bp * LAS_G4D);
      launch_las_dec_cell_bwd(fp(s.dact, (size_t)t * Bp * LAS_G4D), fp(s.dc, (size_t)t * Bp * LAS_HD),
                              t == 0 ? fp(s.cinit) : fp(s.dc, (size_t)(t - 1) * Bp * LAS_HD), fp(s.dHC), fp(s.dhq), fp(s.dS),
                              fp(s.dcd), dGt, Bp, last, st);
      if (int rc = gemm_dense(h, dGt, P + s.off_wah, fp(s.dS), Bp, LAS_SW, LAS_G4D, LAS_G4D, LAS_G4D, LAS_SW, false, true)) return rc;
    }
    launch_las_dec_init_bwd(fp(s.dS), fp(s.dcd), fp(s.dhc), fp(s.dcc), B, Bp, st);
    HIPCHK(h, hipGetLastError());
  }
  {
    PhaseScope ps(h, PH_WGRAD);
    const float* Snext = fp(s.S, (size_t)Bp * LAS_SW);   // rows of steps 1..U: [a_t | h_t]
    if (int rc = gemm_dense(h, Snext, fp(s.dL), G + s.off_wp, LAS_HE, Cp, UB, LAS_SW, Cp, Cp, true, false)) return rc;
    launch_colsum(fp(s.dL), UB, Cp, Cp, G + s.off_bp, fp(s.csws), st);
    if (int rc = gemm_dense(h, fp(s.HC), fp(s.dA), G + s.off_watt, 2 * LAS_HD, LAS_HE, UB, 2 * LAS_HD, LAS_HE, LAS_HE, true, false))
      return rc;
    if (int rc = gemm_dense(h, Snext + LAS_HE, fp(s.dQ), G + s.off_wq, LAS_HD, LAS_HD, UB, LAS_SW, LAS_HD, LAS_HD, true, false))
      return rc;
    launch_colsum(fp(s.dvpart), UB, LAS_HD, LAS_HD, G + s.off_v, fp(s.csws), st);
    if (int rc = gemm_dense(h, fp(s.S), fp(s.dGd), G + s.off_wah, LAS_SW, LAS_G4D, UB, LAS_SW, LAS_G4D, LAS_G4D, true, false))
      return rc;
    launch_colsum(fp(s.dGd), UB, LAS_G4D, LAS_G4D, G + s.off_bd, fp(s.csws), st);
    launch_las_embed_grad(fp(s.dGd), s.ids.as<int32_t>(), U, B, Bp, C, G + s.off_e, st);
    if (int rc = gemm_dense(h, mem, fp(s.dkeys), G + s.off_wmem, LAS_HD, LAS_HD, L4 * Bp, LAS_HD, LAS_HD, LAS_HD, true, false))
      return rc;
    // the memory's gradient: the context's share plus the keys' share, into the top layer's output gradient
    if (int rc = gemm_dense(h, fp(s.dkeys), P + s.off_wmem, fp(s.tmpm), L4 * Bp, LAS_HD, LAS_HD, LAS_HD, LAS_HD, LAS_HD, false, true))
      return rc;
    launch_las_add(fp(s.dmem), LAS_HD, fp(s.tmpm), LAS_HD, fp(s.dout), LAS_HD, L4 * Bp, LAS_HD, st);
    HIPCHK(h, hipGetLastError());
  }
  for (int l = LasEnc::NL - 1; l >= 0; --l) {
    const int L = s.enc.Lr[l];
    const int R = L * Bp;
    {
      PhaseScope ps(h, PH_RECB);
      if (l < LasEnc::NL - 1) {
        HIPCHK(h, hipMemsetAsync(s.dhc.p, 0, (size_t)2 * Bp * LAS_HE * 4, st));
        HIPCHK(h, hipMemsetAsync(s.dcc.p, 0, (size_t)2 * Bp * LAS_HE * 4, st));
      }
      launch_las_transpose_wh(P + s.off_whf[l], fp(s.whT), st);
      launch_las_transpose_wh(P + s.off_whb[l], fp(s.whT, (size_t)LAS_G4E * LAS_HE), st);
      for (int t = L - 1; t >= 0; --t)
        launch_las_enc_bwd_step(fp(s.dout), fp(s.whT), fp(s.whT, (size_t)LAS_G4E * LAS_HE), fp(s.enc.act[l]), fp(s.enc.c[l]), fp(s.dGe), fp(s.dhc),
                                fp(s.dcc), t, L, B, Bp, st);
    }
    PhaseScope ps(h, PH_WGRAD);
    const float* Xin = l == 0 ? h->X0.as<float>() : fp(s.enc.X[l]);
    const int in_rows = (l == 0 ? h->T : s.enc.Lr[l - 1] / 2) * Bp;
    if (int rc = gemm_dense(h, Xin, fp(s.dGe), G + s.off_wx[l], s.Ip[l], 2 * LAS_G4E, R, s.Ip[l], 2 * LAS_G4E, 2 * LAS_G4E, true,
                          false, nullptr, 0, in_rows))
      return rc;
    launch_colsum(fp(s.dGe), R, 2 * LAS_G4E, 2 * LAS_G4E, G + s.off_b[l], fp(s.csws), st);
    // recurrent weights: h of the frame before (fw) / after (bw), zero outside the layer's frames
    const float* o = fp(s.enc.out[l]);
    if (int rc = gemm_dense(h, o, fp(s.dGe), G + s.off_whf[l], LAS_HE, LAS_G4E, R, 2 * LAS_HE, 2 * LAS_G4E, LAS_G4E, true, false,
                          nullptr, -Bp, R))
      return rc;
    if (int rc = gemm_dense(h, o + LAS_HE, fp(s.dGe) + LAS_G4E, G + s.off_whb[l], LAS_HE, LAS_G4E, R, 2 * LAS_HE, 2 * LAS_G4E,
                          LAS_G4E, true, false, nullptr, Bp, R))
      return rc;
    if (l > 0) {
      if (int rc = gemm_dense(h, fp(s.dGe), P + s.off_wx[l], fp(s.dX), R, 4 * LAS_HE, 2 * LAS_G4E, 2 * LAS_G4E, 2 * LAS_G4E,
                            4 * LAS_HE, false, true))
        return rc;
      launch_las_pyr_unpack(fp(s.dX), fp(s.dout), s.enc.Lr[l - 1] / 2, Bp, st);
    }
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, hipEventRecord(h->ev_bucket.back(), st));   // one bucket: the whole gradient with the fault word
  h->have_grads = true;
  return NASR_OK;
}


// ------------------------------------------------------------------ beam search
// host_feats: the search packs features of its own (m.feats, m.X0); otherwise it reads the resident batch's X0
int las_beam_ensure(nasr_ctx* h, LasBeam& m, int B, int T, int W, int max_steps, bool host_feats) {
  const int Bp = rup(B, 16), nrows = B * W, R = rup(nrows, 16), C = h->C;
  bool grew = false, ok = m.enc.ensure(T, Bp, &grew);
  const size_t L4B = (size_t)m.enc.Lr[LasEnc::NL - 1] * Bp, MR = (size_t)max_steps * nrows;
  if (host_feats) {
    ok &= m.feats.ensure((size_t)B * T * h->F * 4, &grew);
    ok &= m.X0.ensure((size_t)T * Bp * h->Fp * 4, &grew);
  }
  ok &= m.keys.ensure(L4B * LAS_HD * 4, &grew);
  ok &= m.S.ensure((size_t)R * LAS_SW * 4, &grew) && m.Sx.ensure((size_t)R * LAS_SW * 4, &grew);
  ok &= m.cs.ensure((size_t)R * LAS_HD * 4, &grew) && m.cx.ensure((size_t)R * LAS_HD * 4, &grew);
  ok &= m.gp.ensure((size_t)R * LAS_G4D * 4, &grew) && m.dact.ensure((size_t)R * LAS_G4D * 4, &grew);
  ok &= m.HC.ensure((size_t)R * 2 * LAS_HD * 4, &grew) && m.Q.ensure((size_t)R * LAS_HD * 4, &grew);
  ok &= m.logits.ensure((size_t)R * h->Cp * 4, &grew) && m.ids.ensure((size_t)R * 4, &grew);
  for (int i = 0; i < 2; ++i)
    ok &= m.logp[i].ensure((size_t)R * 4, &grew) && m.len[i].ensure((size_t)R * 4, &grew) && m.fin[i].ensure((size_t)R * 4, &grew) &&
          m.ctx[i].ensure((size_t)R * 4, &grew);
  ok &= m.scores.ensure((size_t)nrows * C * 4, &grew) && m.totals.ensure((size_t)nrows * C * 4, &grew);
  ok &= m.sel_idx.ensure((size_t)nrows * 4, &grew) && m.sel_score.ensure((size_t)nrows * 4, &grew);
  ok &= m.pen.ensure((size_t)(max_steps + 1) * 4, &grew) && m.flags.ensure(8, &grew);
  ok &= m.tr_score.ensure(MR * 4, &grew) && m.tr_word.ensure(MR * 4, &grew) && m.tr_parent.ensure(MR * 4, &grew);
  ok &= m.gathered.ensure(MR * 4, &grew);
  if (!ok) return h->fail(NASR_ERR_HIP, "hipMalloc failed while sizing beam-search buffers");
  m.B = B; m.Bp = Bp; m.T = T; m.W = W; m.R = R; m.max_steps = max_steps;
  return NASR_OK;
}

// The inference graph of the reference: the encoder, the tiled initial state, then per step the decoder
// cell and attention over all beam rows, the scores and the exact top-W, the update by parent; gather_tree at the end.
// Steps are enqueued in chunks; the host reads the device's done word once per chunk.
// feats: host features [B][T][F], copied and packed into the search's own X0; nullptr: the encoder reads the resident
// batch's time-major X0 (B, T: the resident batch's), which the search only reads.
int las_beam_search(nasr_ctx* h, const float* feats, int B, int T, int W, int max_steps, int start_id, int end_id, float lp) {
  LasState& s = *h->las;
  if (!s.beam) s.beam.reset(new LasBeam());
  LasBeam& m = *s.beam;
  m.have = false;
  if (int rc = las_beam_ensure(h, m, B, T, W, max_steps, feats != nullptr)) return rc;
  const int Bp = m.Bp, R = m.R, nrows = B * W, C = h->C, Cp = h->Cp;
  const int L4 = m.enc.Lr[LasEnc::NL - 1];
  const float* P = h->P;
  hipStream_t st = h->st;
  const bool timed = h->profiling;
  m.marks.clear();
  size_t nev = 0;
  const std::function<void(int)> mark = [&](int ph) {
    if (!timed) return;
    if (nev == m.ev.size()) (void)hipEventCreate(m.ev.emplace_back().out());
    (void)hipEventRecord(m.ev[nev], st);
    m.marks.push_back({ph, nev++});
  };
  // (5 + n)^lp / 6^lp in fp32 for every length a step can see (TF: 1 when lp is 0)
  m.hpen.assign((size_t)max_steps + 1, 1.f);
  if (lp != 0.f)
    for (int n = 0; n <= max_steps; ++n) m.hpen[n] = powf(5.f + (float)n, lp) / powf(6.f, lp);
  mark(-1);
  HIPCHK(h, hipMemcpyAsync(m.pen.p, m.hpen.data(), m.hpen.size() * 4, hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemsetAsync(m.flags.p, 0, 8, st));
  if (feats) {
    HIPCHK(h, hipMemcpyAsync(m.feats.p, feats, (size_t)B * T * h->F * 4, hipMemcpyHostToDevice, st));
    launch_pack_feats(m.feats.as<float>(), m.X0.as<float>(), B, Bp, T, h->F, h->Fp, st);
  }
  const float* X0 = feats ? m.X0.as<float>() : h->X0.as<float>();
  if (int rc = las_encode(h, X0, T, B, m.enc)) return rc;
  // the n-gram table, if one is set: every row's context starts as start_id in every digit
  const float* table = s.lm_order ? fp(s.lm) : nullptr;
  const int K = s.lm_order ? s.lm_K : 1;
  int ctx0 = 0;
  for (int d = 1; d < s.lm_order; ++d) ctx0 = ctx0 * C + start_id;
  const float* mem = fp(m.enc.out[LasEnc::NL - 1]);
  if (int rc = gemm_dense(h, mem, P + s.off_wmem, fp(m.keys), L4 * Bp, LAS_HD, LAS_HD, LAS_HD, LAS_HD, LAS_HD, false, false))
    return rc;
  launch_las_beam_init(mem, fp(m.enc.c[LasEnc::NL - 1]), L4, Bp, W, nrows, R, start_id, fp(m.S), fp(m.cs), m.ids.as<int32_t>(),
                       fp(m.logp[0]), m.len[0].as<int32_t>(), m.fin[0].as<int32_t>(), m.ctx[0].as<int32_t>(), ctx0, st);
  HIPCHK(h, hipGetLastError());
  mark(LB_ENC);
  const int32_t* done = m.flags.as<int32_t>();
  int32_t hf[2] = {0, 0};
  constexpr int CHUNK = 8;
  // every step reads the beams' S / cs and writes Sx / cx, which the update gathers by parent back into S / cs
  LasStep step{};
  step.S = fp(m.S); step.ids = m.ids.as<int32_t>(); step.cprev = fp(m.cs);
  step.gp = fp(m.gp); step.act = fp(m.dact); step.c = fp(m.cx); step.Snext = fp(m.Sx);
  step.HC = fp(m.HC); step.Q = fp(m.Q); step.logits = fp(m.logits);
  step.keys = fp(m.keys); step.mem = mem; step.L4 = L4; step.Bp = Bp; step.W = W; step.nrows = nrows;
  step.done = done;
  for (int t = 0; t < max_steps;) {
    for (const int end = std::min(max_steps, t + CHUNK); t < end; ++t) {
      const int i = t & 1, o = i ^ 1;
      const size_t tr = (size_t)t * nrows;
      if (int rc = las_decoder_step(h, R, step, mark)) return rc;
      launch_las_beam_score(fp(m.logits), Cp, C, fp(m.logp[i]), m.len[i].as<int32_t>(), m.fin[i].as<int32_t>(), fp(m.pen), end_id,
                            nrows, table, m.ctx[i].as<int32_t>(), s.lm_weight, fp(m.scores), fp(m.totals), done, st);
      launch_las_beam_select(fp(m.scores), B, W, C, m.sel_idx.as<int32_t>(), fp(m.sel_score), done, st);
      launch_las_beam_update(m.sel_idx.as<int32_t>(), fp(m.sel_score), fp(m.totals), W, C, end_id, nrows, fp(m.Sx), fp(m.cx),
                             m.len[i].as<int32_t>(), m.fin[i].as<int32_t>(), m.ctx[i].as<int32_t>(), K, fp(m.S), fp(m.cs),
                             m.ids.as<int32_t>(), fp(m.logp[o]), m.len[o].as<int32_t>(), m.fin[o].as<int32_t>(),
                             m.ctx[o].as<int32_t>(), fp(m.tr_score) + tr,
                             m.tr_word.as<int32_t>() + tr, m.tr_parent.as<int32_t>() + tr, done, st);
      launch_las_beam_finish(m.fin[o].as<int32_t>(), nrows, t, max_steps, m.flags.as<int32_t>(), st);
      HIPCHK(h, hipGetLastError());
      mark(LB_SEL);
    }
    HIPCHK(h, hipMemcpyAsync(hf, m.flags.p, 8, hipMemcpyDeviceToHost, st));
    if (int rc = sync_checked(h)) return rc;
    mark(LB_WAIT);
    if (hf[0]) break;
  }
  m.Tdec = hf[1];
  m.end_id = end_id;
  if (m.Tdec < 1 || m.Tdec > max_steps) return h->fail(NASR_ERR_HIP, "las beam search: the device's step count is out of range");
  launch_las_beam_gather_tree(m.tr_word.as<int32_t>(), m.tr_parent.as<int32_t>(), m.len[m.Tdec & 1].as<int32_t>(), m.Tdec, B, W,
                              end_id, m.gathered.as<int32_t>(), st);
  HIPCHK(h, hipGetLastError());
  mark(LB_TREE);
  if (int rc = sync_checked(h)) return rc;
  m.timed = timed;
  if (timed) {
    for (float& x : m.times) x = 0.f;
    for (size_t k = 1; k < m.marks.size(); ++k) {
      float ms = 0.f;
      HIPCHK(h, hipEventElapsedTime(&ms, m.ev[m.marks[k - 1].second], m.ev[m.marks[k].second]));
      m.times[m.marks[k].first] += ms;
    }
  }
  m.have = true;
  return NASR_OK;
}

}  // namespace nasr_impl

void nasr_impl::LasStateDelete::operator()(LasState* s) const { delete s; }

namespace {
// [U][Bp][cols] (element size esz) read back and reordered to [B][U][cols]
int las_read_bu(nasr_ctx* h, const DevBuf& src, int cols, int ld, size_t esz, void* dst) {
  LasState& s = *h->las;
  const int B = h->B, Bp = h->Bp, U = s.U;
  std::vector<char> tmp((size_t)U * Bp * ld * esz);
  HIPCHK(h, hipMemcpyAsync(tmp.data(), src.p, tmp.size(), hipMemcpyDeviceToHost, h->st));
  if (int rc = sync_checked(h)) return rc;
  char* d = static_cast<char*>(dst);
  for (int b = 0; b < B; ++b)
    for (int t = 0; t < U; ++t)
      memcpy(d + ((size_t)b * U + t) * cols * esz, tmp.data() + ((size_t)t * Bp + b) * ld * esz, (size_t)cols * esz);
  return NASR_OK;
}
}  // namespace

extern "C" {

int nasr_create_las(const nasr_las_cfg* cfg, int device_id, void* stream, nasr_handle* out) {
  if (!cfg || !out) {
    g_create_error = "nasr_create_las: null argument";
    return NASR_ERR_ARG;
  }
  *out = nullptr;
  if (cfg->feature_size < 1 || cfg->num_classes < 2) {
    g_create_error = "nasr_create_las: feature_size must be >= 1 and num_classes >= 2";
    return NASR_ERR_ARG;
  }
  if (cfg->num_hidden != LAS_H || cfg->num_layers != LasEnc::NL) {
    g_create_error = "nasr_create_las: only num_hidden = 250 and num_layers = 4 (the reference's) are implemented";
    return NASR_ERR_ARG;
  }
  if (!(cfg->sampling_probability >= 0.f && cfg->sampling_probability <= 1.f)) {
    g_create_error = "nasr_create_las: sampling_probability must be in [0,1]";
    return NASR_ERR_ARG;
  }
  nasr_ctx* h = nullptr;
  if (int rc = handle_open("nasr_create_las", Family::Las, device_id, stream, &h, nullptr)) return rc;
  h->beta1 = cfg->beta1; h->beta2 = cfg->beta2; h->epsilon = cfg->epsilon;
  h->lr = cfg->learning_rate;
  h->graph_mode = false;
  h->las.reset(new LasState());
  LasState& s = *h->las;
  s.cfg = *cfg;
  s.p = cfg->sampling_probability;
  s.seed = cfg->seed;
  las_layout(h);
  if (!alloc_param_buffers(h)) return create_fail(h, NASR_ERR_HIP, "hipMalloc of parameter buffers failed");
  h->buckets.push_back({0, GRAD_HEAD + h->np_int});   // one bucket: the whole gradient, complete at the end of the backward pass
  if (int rc = handle_finish(h)) return rc;
  *out = h;
  return NASR_OK;
}

int nasr_las_set_sampling(nasr_handle h, float p, uint32_t seed, uint32_t counter, int tower) {
  LAS_CALL(h);
  LasState* s = h->las.get();
  if (!(p >= 0.f && p <= 1.f) || tower < 0) return h->fail(NASR_ERR_ARG, "nasr_las_set_sampling: p must be in [0,1], tower >= 0");
  s->p = p; s->seed = seed; s->counter = counter; s->tower = tower;
  return NASR_OK;
}

int nasr_las_get_sampling(nasr_handle h, float* p, uint32_t* seed, uint32_t* counter, int* tower) {
  LAS_CALL(h);
  LasState* s = h->las.get();
  if (p) *p = s->p;
  if (seed) *seed = s->seed;
  if (counter) *counter = s->counter;
  if (tower) *tower = s->tower;
  return NASR_OK;
}

namespace {
// the decoder pass of nasr_las_forward / nasr_las_forward_resident on the resident batch
int las_forward_out(nasr_ctx* h, int sample, float* logits_out) {
  if (int rc = las_forward(h, sample != 0)) return rc;
  if (logits_out) return nasr_las_get_logits(h, logits_out);
  return sync_checked(h);
}
}  // namespace

int nasr_las_forward(nasr_handle h, const float* feats, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len,
                     int B, int T, int U, int sample, float* logits_out) {
  LAS_CALL(h);
  if (!labels || !label_len) return h->fail(NASR_ERR_ARG, "nasr_las_forward needs labels");
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = upload(h, stacked_batch(feats, seq_len, labels, label_len, B, T, U))) return rc;
  return las_forward_out(h, sample, logits_out);
}

int nasr_las_forward_resident(nasr_handle h, int sample, float* logits_out) {
  LAS_CALL(h);
  if (!h->resident) return h->fail(NASR_ERR_STATE, "nasr_las_forward_resident: no resident batch");
  HIPCHK(h, hipSetDevice(h->device));
  return las_forward_out(h, sample, logits_out);
}

int nasr_las_get_logits(nasr_handle h, float* logits_out) {
  LAS_CALL(h);
  LasState* s = h->las.get();
  if (!logits_out) return h->fail(NASR_ERR_ARG, "nasr_las_get_logits: null output");
  if (!s->have_pass) return h->fail(NASR_ERR_STATE, "nasr_las_get_logits: no decoder pass has run");
  return las_read_bu(h, s->logits, h->C, h->Cp, 4, logits_out);
}

int nasr_las_get_fed_ids(nasr_handle h, int32_t* ids_out) {
  LAS_CALL(h);
  LasState* s = h->las.get();
  if (!ids_out) return h->fail(NASR_ERR_ARG, "nasr_las_get_fed_ids: null output");
  if (!s->have_pass) return h->fail(NASR_ERR_STATE, "nasr_las_get_fed_ids: no decoder pass has run");
  return las_read_bu(h, s->ids, 1, 1, 4, ids_out);
}

int nasr_las_get_sampled(nasr_handle h, int32_t* sampled_out) {
  LAS_CALL(h);
  LasState* s = h->las.get();
  if (!sampled_out) return h->fail(NASR_ERR_ARG, "nasr_las_get_sampled: null output");
  if (!s->have_pass) return h->fail(NASR_ERR_STATE, "nasr_las_get_sampled: no decoder pass has run");
  return las_read_bu(h, s->sampled, 1, 1, 4, sampled_out);
}

namespace {
// The argument ranges of a search and the search itself.  feats: host features, or nullptr for the resident batch's X0;
// seq_len: the host's copy of the batch's lengths.
int las_beam_call(nasr_ctx* h, const std::string& fn, const float* feats, const int32_t* seq_len, int B, int T, int beam_width,
                  int max_steps, int start_id, int end_id, float length_penalty, int32_t* steps_out) {
  if (B < 1 || B > 64 || T < 1) return h->fail(NASR_ERR_ARG, fn + ": B must be in [1,64] and T >= 1");
  for (int b = 0; b < B; ++b)
    if (seq_len[b] < 1 || seq_len[b] > T) return h->fail(NASR_ERR_ARG, fn + ": seq_len[" + std::to_string(b) + "] out of [1,T]");
  if (beam_width < 1 || beam_width > 1024) return h->fail(NASR_ERR_ARG, fn + ": beam_width must be in [1,1024]");
  if (max_steps < 1 || max_steps > 1000) return h->fail(NASR_ERR_ARG, fn + ": max_steps must be in [1,1000]");
  if (start_id < 0 || start_id >= h->C || end_id < 0 || end_id >= h->C)
    return h->fail(NASR_ERR_ARG, fn + ": start_id and end_id must be in [0, num_classes-1]");
  if (!(length_penalty >= 0.f) || !std::isfinite(length_penalty))
    return h->fail(NASR_ERR_ARG, fn + ": length_penalty must be finite and >= 0");
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = las_beam_search(h, feats, B, T, beam_width, max_steps, start_id, end_id, length_penalty)) return rc;
  if (steps_out) *steps_out = h->las->beam->Tdec;
  return NASR_OK;
}
}  // namespace

int nasr_las_beam_search(nasr_handle h, const float* feats, const int32_t* seq_len, int B, int T, int beam_width, int max_steps,
                         int start_id, int end_id, float length_penalty, int32_t* steps_out) {
  LAS_CALL(h);
  if (!feats || !seq_len) return h->fail(NASR_ERR_ARG, "nasr_las_beam_search: null input buffer");
  return las_beam_call(h, "nasr_las_beam_search", feats, seq_len, B, T, beam_width, max_steps, start_id, end_id, length_penalty,
                       steps_out);
}

int nasr_las_beam_search_resident(nasr_handle h, int beam_width, int max_steps, int start_id, int end_id, float length_penalty,
                                  int32_t* steps_out) {
  LAS_CALL(h);
  if (!h->resident) return h->fail(NASR_ERR_STATE, "nasr_las_beam_search_resident: no resident batch");
  return las_beam_call(h, "nasr_las_beam_search_resident", nullptr, h->h_seq.data(), h->B, h->T, beam_width, max_steps, start_id,
                       end_id, length_penalty, steps_out);
}

namespace {
// the last search's buffers of a LAS handle (after LAS_CALL), or nullptr with *rc set
LasBeam* beam_of(nasr_handle h, const char* fn, int* rc) {
  LasBeam* m = h->las->beam.get();
  *rc = m && m->have ? NASR_OK : h->fail(NASR_ERR_STATE, std::string(fn) + ": no beam search has run");
  return *rc ? nullptr : m;
}
// [Tdec][B*W] read back and reordered to [B][Tdec][W]
int beam_read_tbw(nasr_ctx* h, const LasBeam& m, const DevBuf& src, void* dst) {
  const int B = m.B, W = m.W, Td = m.Tdec, n = B * W;
  std::vector<int32_t> tmp((size_t)Td * n);
  HIPCHK(h, hipMemcpyAsync(tmp.data(), src.p, tmp.size() * 4, hipMemcpyDeviceToHost, h->st));
  if (int rc = sync_checked(h)) return rc;
  int32_t* d = static_cast<int32_t*>(dst);
  for (int b = 0; b < B; ++b)
    for (int t = 0; t < Td; ++t) memcpy(d + ((size_t)b * Td + t) * W, tmp.data() + (size_t)t * n + (size_t)b * W, (size_t)W * 4);
  return NASR_OK;
}
int beam_read(nasr_ctx* h, const DevBuf& src, size_t n, void* dst) {
  HIPCHK(h, hipMemcpyAsync(dst, src.p, n * 4, hipMemcpyDeviceToHost, h->st));
  return sync_checked(h);
}
}  // namespace

int nasr_las_beam_get_ids(nasr_handle h, int32_t* ids_out) {
  LAS_CALL(h);
  int rc;
  LasBeam* m = beam_of(h, __func__, &rc);
  if (!m) return rc;
  if (!ids_out) return h->fail(NASR_ERR_ARG, "nasr_las_beam_get_ids: null output");
  return beam_read_tbw(h, *m, m->gathered, ids_out);
}

int nasr_las_beam_get_trace(nasr_handle h, float* scores_out, int32_t* word_out, int32_t* parent_out) {
  LAS_CALL(h);
  int rc;
  LasBeam* m = beam_of(h, __func__, &rc);
  if (!m) return rc;
  if (scores_out && (rc = beam_read_tbw(h, *m, m->tr_score, scores_out))) return rc;
  if (word_out && (rc = beam_read_tbw(h, *m, m->tr_word, word_out))) return rc;
  if (parent_out && (rc = beam_read_tbw(h, *m, m->tr_parent, parent_out))) return rc;
  return NASR_OK;
}

int nasr_las_beam_get_final(nasr_handle h, float* log_probs_out, int32_t* lengths_out, int32_t* finished_out) {
  LAS_CALL(h);
  int rc;
  LasBeam* m = beam_of(h, __func__, &rc);
  if (!m) return rc;
  const int f = m->Tdec & 1;
  const size_t n = (size_t)m->B * m->W;
  if (log_probs_out && (rc = beam_read(h, m->logp[f], n, log_probs_out))) return rc;
  if (lengths_out && (rc = beam_read(h, m->len[f], n, lengths_out))) return rc;
  if (finished_out && (rc = beam_read(h, m->fin[f], n, finished_out))) return rc;
  return NASR_OK;
}

int nasr_las_beam_set_lm(nasr_handle h, const float* logp, int order, float weight) {
  LAS_CALL(h);
  LasState* s = h->las.get();
  if (logp) {
    if (order < 1 || order > 4) return h->fail(NASR_ERR_ARG, "nasr_las_beam_set_lm: order must be in [1,4]");
    if (!std::isfinite(weight)) return h->fail(NASR_ERR_ARG, "nasr_las_beam_set_lm: weight must be finite");
  }
  const int64_t C = h->C, lim = (int64_t)1 << 24;
  int64_t K = 1;
  for (int d = 1; logp && d < order && K * C <= lim; ++d) K *= C;
  if (K * C > lim) return h->fail(NASR_ERR_ARG, "nasr_las_beam_set_lm: a table of num_classes^order entries exceeds 2^24");
  if (logp)   // (0 * -inf is NaN: a non-finite entry would break "weight 0 is the plain search")
    for (int64_t i = 0; i < K * C; ++i)
      if (!std::isfinite(logp[i])) return h->fail(NASR_ERR_ARG, "nasr_las_beam_set_lm: every table entry must be finite");
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = sync_checked(h)) return rc;   // (a search in flight may still read the table this call replaces or frees)
  // the handle is on the plain search from here until the new table is whole on the device
  s->lm_order = 0; s->lm_K = 1; s->lm_weight = 0.f;
  if (!logp) {
    s->lm.release();
    return NASR_OK;
  }
  if (!s->lm.ensure((size_t)(K * C) * 4, nullptr)) return h->fail(NASR_ERR_HIP, "nasr_las_beam_set_lm: hipMalloc failed");
  HIPCHK(h, hipMemcpyAsync(s->lm.p, logp, (size_t)(K * C) * 4, hipMemcpyHostToDevice, h->st));
  if (int rc = sync_checked(h)) return rc;
  s->lm_order = order; s->lm_K = (int)K; s->lm_weight = weight;
  return NASR_OK;
}

int nasr_las_beam_get_lm_context(nasr_handle h, int32_t* ctx_out) {
  LAS_CALL(h);
  int rc;
  LasBeam* m = beam_of(h, __func__, &rc);
  if (!m) return rc;
  if (!ctx_out) return h->fail(NASR_ERR_ARG, "nasr_las_beam_get_lm_context: null output");
  return beam_read(h, m->ctx[m->Tdec & 1], (size_t)m->B * m->W, ctx_out);
}

int nasr_las_beam_get_times(nasr_handle h, float* ms_out) {
  LAS_CALL(h);
  int rc;
  LasBeam* m = beam_of(h, __func__, &rc);
  if (!m) return rc;
  if (!ms_out) return h->fail(NASR_ERR_ARG, "nasr_las_beam_get_times: null output");
  if (!m->timed) return h->fail(NASR_ERR_STATE, "nasr_las_beam_get_times: the last search ran with profiling off");
  memcpy(ms_out, m->times, sizeof(m->times));
  return NASR_OK;
}

}  // extern "C"
