// nasr_batch.hip — the batch side of a handle: HBM buffers sized to the batch shape, input validation, and the batch slots
// (synchronous upload, staging through pinned memory on the copy stream, commit).  Replaces the feed_dict of
// TensorFlowNetwork.train (networks/tfnetwork.py:183-190) and DataSet.get_next_batch's hand-over (dataset.py:33-40).
#include "nasr_lstm.h"

using namespace nasr;
using namespace nasr_impl;

namespace nasr_impl {

int ensure_ctc_buffers(nasr_ctx* h, int B, int Bp, int T, int Tp, int Lmax, bool* grew) {
  const int KSa = ctc_states_per_lane(Lmax);
  if (KSa > 16) return h->fail(NASR_ERR_ARG, "label length > 511 not supported by the CTC lattice kernel");
  // the plain walk of ctc.hip (2) gathers its emissions at 32-bit BYTE offsets from the utterance's first row
  if ((size_t)Tp * Bp * h->Cp * 4 >= ((size_t)1 << 32))
    return h->fail(NASR_ERR_ARG, "T' x B x C logits beyond the lattice kernels' 32-bit offsets: " + std::to_string(Tp) + " x " +
                                     std::to_string(Bp) + " x " + std::to_string(h->Cp) + " floats");
  bool ok = true;
  ok &= h->logits.ensure((size_t)Tp * Bp * h->Cp * 4, grew);
  ok &= h->logz.ensure((size_t)Tp * Bp * 4, grew);
  ok &= h->alpha.ensure((size_t)B * (T + 8) * KSa * 64 * 4, grew);
  ok &= h->beta.ensure((size_t)B * (T + 8) * KSa * 64 * 4, grew);
  ok &= h->aoff.ensure((size_t)B * (T + 8) * 8, grew);
  ok &= h->boff.ensure((size_t)B * (T + 8) * 8, grew);
  ok &= h->logp.ensure((size_t)Bp * 8, grew);
  ok &= h->ctcprobs.ensure((size_t)Tp * Bp * h->Cp * 4, grew);              // emission rows of the CTC lattice (ctc.hip (2b))
  ok &= h->ctckexp.ensure((size_t)B * 2 * ctc_group_rows(T + 8) * 8, grew);   // its column offsets per group of frames
  ok &= h->nll.ensure((size_t)Bp * 4, grew);
  ok &= h->loss.ensure(16, grew);
  ok &= h->amax.ensure((size_t)Tp * Bp * 4, grew);
  ok &= h->ids.ensure((size_t)B * Tp * 4, grew);
  ok &= h->lens.ensure((size_t)Bp * 4, grew);
  if (!ok) return h->fail(NASR_ERR_HIP, "hipMalloc failed while sizing batch buffers");
  return KSa;
}

int ensure_shape(nasr_ctx* h, int B, int T, int Lmax, bool chunked) {
  switch (h->family) {
    case Family::WaveNet: return wn_ensure_shape(h, B, T, Lmax);
    case Family::Las: return las_ensure_shape(h, B, T, Lmax);
    default: return lstm_ensure_shape(h, B, T, Lmax, chunked);
  }
}

int lstm_ensure_shape(nasr_ctx* h, int B, int T, int Lmax, bool chunked) {
  LstmState* const ls = h->lstm.get();
  const int Bp = rup(B, 16);
  const int Tp = lstm_logit_frames(h, T);
  // the LSTM stack's time axis: the batch's frames, or the rows of its windows
  LcGeom lg{};
  if (chunked) {
    lg.C = ls->lcC; lg.W = std::min(ls->lcC + ls->lcR, T); lg.K = lc_last_window(T, lg.C, lg.W) + 1; lg.T = T; lg.Bp = Bp;
    if ((int64_t)lg.K * lg.W * Bp > ((int64_t)1 << 22))
      return h->fail(NASR_ERR_ARG, "chunked batch: " + std::to_string(lg.K) + " windows of " + std::to_string(lg.W) + " rows x " +
                                       std::to_string(Bp) + " utterances are more than 2^22 rows: use a longer chunk or a shorter look-ahead");
  }
  const int Tv = chunked ? lg.K * lg.W : T;
  const size_t R = (size_t)Tv * Bp;
  const int D = ls->D, Hp = ls->Hp, N4 = ls->N4;
  bool grew = false;
  bool ok = true;
  const int KSa = ensure_ctc_buffers(h, B, Bp, T, Tp, Lmax, &grew);
  if (KSa < 0) return KSa;
  ok &= h->X0.ensure(R * h->Fp * 4, &grew);
  if (chunked) {
    ok &= ls->lc_x0.ensure((size_t)T * Bp * h->Fp * 4, &grew);
    ok &= ls->lc_top.ensure((size_t)T * Bp * ls->Pinp * 4, &grew) && ls->lc_dtop.ensure((size_t)T * Bp * ls->Pinp * 4, &grew);
    ok &= ls->lc_cimg.ensure((size_t)D * Bp * Hp * 4, &grew) && ls->lc_dcc.ensure((size_t)Bp * Hp * 4, &grew);
  }
  ok &= h->seqbuf.ensure((size_t)Bp * 4, &grew);
  ok &= ls->dout.ensure(R * D * Hp * 4, &grew);
  ok &= ls->hstate.ensure((size_t)2 * D * Bp * Hp * 4, &grew);
  ok &= ls->partial.ensure((size_t)2 * D * (Hp / 32) * Bp * Hp * 4, &grew);
  ok &= ls->dcstate.ensure((size_t)2 * D * Bp * Hp * 4, &grew);
  ok &= ls->dgbuf.ensure(R * D * N4 * 4, &grew);
  if (ls->rec_kind == RecKind::Persist) ok &= ls->dgmax.ensure(persist_dgmax_floats(T, Bp, Hp, D) * 4, &grew);
  {
    int ipmax = h->Fp, wmax = D * N4;
    for (int l = 0; l < ls->L; ++l) ipmax = std::max(ipmax, ls->Ip[l]);
    for (int i = 0; i < ls->ndense; ++i) { ipmax = std::max(ipmax, ls->dIp[i]); wmax = std::max(wmax, ls->dWp[i]); }
    ok &= ls->XTP.ensure(tph_bytes((int)R, ipmax), &grew);
    ok &= ls->X0TTP.ensure(tph_bytes(ls->Ip[0], (int)R), &grew);
    for (int l = 0; l < ls->L; ++l) ok &= ls->OTT[l].ensure(tph_bytes(D * Hp, (int)R), &grew);
    ok &= ls->GTP.ensure(tph_bytes((int)R, wmax), &grew);
    ok &= ls->GTTP.ensure(tph_bytes(wmax, (int)R), &grew);
    if (ls->wg_overlap) {
      ok &= ls->GTTP2.ensure(tph_bytes(wmax, (int)R), &grew);
      ok &= ls->sc_gc2.ensure((size_t)wmax);
    }
    if (ls->ndense) ok &= ls->DTP.ensure(tph_bytes(ipmax, (int)R), &grew);
    {
      const size_t n15 = std::max<size_t>(R, (size_t)std::max(ipmax, wmax));
      if (n15 > ls->sc15_n) {
        ok &= ls->sc15.ensure(n15);
        if (ok) {
          launch_fill(ls->sc15.sp(), 32768.f, (int)n15, h->st);
          launch_fill(ls->sc15.ip(), 1.f / 32768.f, (int)n15, h->st);
          ls->sc15_n = n15;
        }
      }
      ok &= ls->sc_x0r.ensure(R) && ls->sc_x0c.ensure((size_t)h->Fp);
      ok &= ls->sc_gr.ensure(R) && ls->sc_gc.ensure((size_t)wmax);
      if (ls->compactable || chunked) {
        ok &= ls->sc_cr.ensure(R + 64) && ls->sc_cx.ensure(R + 64);
        ok &= ls->OTS.ensure((ls->wg_overlap ? 2 : 1) * tph_bytes(D * Hp, (int)R), &grew);
      }
      for (int i = 0; i < ls->ndense; ++i) ok &= ls->sc_yr[i].ensure(R) && ls->sc_yc[i].ensure((size_t)ls->dWp[i]);
      bool g2 = false;
      ok &= ls->scws.ensure(tph_scale_ws_floats((int)R, std::max(ipmax, wmax)) * 4, &g2);
    }
  }
  int csw = std::max(D * N4, h->Cp);
  for (int i = 0; i < ls->ndense; ++i) csw = std::max(csw, ls->dWp[i]);
  // column-sum partials: 32 rows of launch_colsum, or the 64-row partials of the split pass (tp_split2_parts)
  ok &= ls->csws.ensure((size_t)std::max(32, tp_split2_parts((int)R)) * csw * 4, &grew);
  if (ls->wg_overlap) ok &= ls->csws2.ensure((size_t)std::max(32, tp_split2_parts((int)R)) * csw * 4, &grew);
  for (int i = 0; i < ls->ndense; ++i) {
    ok &= ls->Ybuf[i].ensure(R * ls->dWp[i] * 4, &grew);
    ok &= ls->dYbuf[i].ensure(R * ls->dWp[i] * 4, &grew);
  }
  for (int l = 0; l < ls->L; ++l) {
    ok &= ls->gates[l].ensure(R * D * N4 * 4, &grew);
    ok &= ls->outb[l].ensure(R * D * Hp * 4, &grew);
    ok &= ls->cbuf[l].ensure(R * D * Hp * 4, &grew);
  }
  if (!ok) return h->fail(NASR_ERR_HIP, "hipMalloc failed while sizing batch buffers");
  if (grew || Bp != h->Bp) drop_graphs(h);
  h->B = B; h->Bp = Bp; h->T = T; h->Lmax = Lmax; h->Tp = Tp; h->KS = KSa;
  ls->Tv = Tv; ls->lc_live = chunked; ls->lcg = lg;
  return NASR_OK;
}

int validate_batch(nasr_ctx* h, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T,
                   int Lmax, int num_classes, int skip) {
  const bool las = !num_classes && h->family == Family::Las;
  const int C = num_classes ? num_classes : h->C;
  if (B < 1 || B > 64) return h->fail(NASR_ERR_ARG, "per-GPU batch must be in [1,64]");
  if (T < 1) return h->fail(NASR_ERR_ARG, "T must be >= 1");
  for (int b = 0; b < B; ++b) {
    if (seq_len[b] < 1 || seq_len[b] > T)
      return h->fail(NASR_ERR_ARG, "seq_len[" + std::to_string(b) + "] out of [1,T]");
    if (!labels) continue;
    if (las) {   // dense labels: every entry is fed to the decoder, any class is a label, no CTC feasibility
      if (label_len[b] < 0 || label_len[b] > Lmax)
        return h->fail(NASR_ERR_ARG, "label_len[" + std::to_string(b) + "] out of [0,Lmax]");
      for (int i = 0; i < Lmax; ++i) {
        const int v = labels[(size_t)b * Lmax + i];
        if (v < 0 || v >= C) return h->fail(NASR_ERR_ARG, "label id out of [0, num_classes-1]");
      }
      continue;
    }
    const int L = label_len[b];
    if (L < 0 || L > Lmax) return h->fail(NASR_ERR_ARG, "label_len[" + std::to_string(b) + "] out of [0,Lmax]");
    int rep = 0;
    for (int i = 0; i < L; ++i) {
      const int v = labels[(size_t)b * Lmax + i];
      if (v < 0 || v >= C - 1)
        return h->fail(NASR_ERR_ARG, "label id out of [0, num_classes-2] (blank = num_classes-1 is not a label)");
      if (i > 0 && v == labels[(size_t)b * Lmax + i - 1]) ++rep;
    }
    const int avail = skip_frames(seq_len[b], skip);
    if (L + rep > avail)
      return h->fail(NASR_ERR_INFEASIBLE, "Not enough time for target transition sequence (required: " +
                                              std::to_string(L + rep) + ", available: " + std::to_string(avail) +
                                              (skip > 1 ? " network frames: " + std::to_string(seq_len[b]) + " input frames under frame_skip " +
                                                              std::to_string(skip)
                                                        : std::string()) +
                                              ") in sequence " + std::to_string(b));
  }
  return NASR_OK;
}

int validate_chunk(nasr_ctx* h, const int32_t* n_frames, int S, int Tc) {
  if (Tc < 1) return h->fail(NASR_ERR_ARG, "a stream chunk needs Tc >= 1");
  for (int b = 0; b < S; ++b)
    if (n_frames[b] < 0 || n_frames[b] > Tc)
      return h->fail(NASR_ERR_ARG, "n_frames[" + std::to_string(b) + "] = " + std::to_string(n_frames[b]) + " out of [0,Tc = " +
                                       std::to_string(Tc) + "]");
  return NASR_OK;
}

// The checks of nasr_batch_aug (include/nasr.h) against the batch's own seq_len; *masked: some mask has a non-zero width.
static int validate_aug(nasr_ctx* h, const nasr_batch_aug* a, const int32_t* seq_len, int B, int ctx, int ncep, bool* masked) {
  *masked = false;
  if (a->n_time < 0 || a->n_time > NASR_AUG_MAX_MASKS || a->n_freq < 0 || a->n_freq > NASR_AUG_MAX_MASKS)
    return h->fail(NASR_ERR_ARG, "augmentation: n_time = " + std::to_string(a->n_time) + ", n_freq = " + std::to_string(a->n_freq) +
                                     ": each must be in [0," + std::to_string(NASR_AUG_MAX_MASKS) + "]");
  if (a->static_width < 1 || ncep % a->static_width)
    return h->fail(NASR_ERR_ARG, "augmentation: static_width " + std::to_string(a->static_width) + " does not divide the frame width " +
                                     std::to_string(ncep));
  if ((a->n_time && !a->time_mask) || (a->n_freq && !a->freq_mask)) return h->fail(NASR_ERR_ARG, "augmentation: null mask array");
  if (2 * (int64_t)ctx + 1 + ncep > 32768) return h->fail(NASR_ERR_ARG, "augmentation: 2*numcontext+1 + frame width > 32768");
  for (int b = 0; b < B; ++b) {
    for (int k = 0; k < a->n_time; ++k) {
      const int64_t t0 = a->time_mask[((size_t)b * a->n_time + k) * 2], tw = a->time_mask[((size_t)b * a->n_time + k) * 2 + 1];
      if (t0 < 0 || tw < 0 || t0 + tw > seq_len[b])
        return h->fail(NASR_ERR_ARG, "augmentation: time mask " + std::to_string(k) + " of utterance " + std::to_string(b) + " [" +
                                         std::to_string(t0) + ", " + std::to_string(t0 + tw) + ") is not inside its " +
                                         std::to_string(seq_len[b]) + " frames");
      *masked |= tw > 0;
    }
    for (int k = 0; k < a->n_freq; ++k) {
      const int64_t f0 = a->freq_mask[((size_t)b * a->n_freq + k) * 2], fw = a->freq_mask[((size_t)b * a->n_freq + k) * 2 + 1];
      if (f0 < 0 || fw < 0 || f0 + fw > a->static_width)
        return h->fail(NASR_ERR_ARG, "augmentation: frequency mask " + std::to_string(k) + " of utterance " + std::to_string(b) + " [" +
                                         std::to_string(f0) + ", " + std::to_string(f0 + fw) + ") is not inside the static block of " +
                                         std::to_string(a->static_width) + " columns");
      *masked |= fw > 0;
    }
  }
  return NASR_OK;
}

bool pinned_ensure(Pinned<void>& p, size_t* cap, size_t bytes) {
  if (bytes <= *cap) return true;
  *cap = 0;
  const size_t want = bytes + bytes / 8;
  if (hipHostMalloc(p.out(), want, hipHostMallocMapped) != hipSuccess) return false;   // (kernels write step results into it)
  *cap = want;
  return true;
}

// Takes a free slot (round robin), marks it FILLING.  NULL when every slot holds a staged or the resident batch.
BatchSlot* slot_acquire(nasr_ctx* h, bool for_stage) {
  std::lock_guard<std::mutex> lk(h->slot_mu);
  if (for_stage) {   // staged batches never take the slot a synchronous upload (validate, decode, ...) needs
    int ahead = 0;
    for (const BatchSlot& s : h->slots) ahead += s.state == SLOT_STAGED || s.state == SLOT_FILLING;
    if (ahead >= NSTAGE) return nullptr;
  }
  for (int k = 0; k < NSLOT; ++k) {
    BatchSlot& s = h->slots[(h->slot_rr + k) % NSLOT];
    if (s.state == SLOT_FREE) {
      h->slot_rr = (h->slot_rr + k + 1) % NSLOT;
      s.state = SLOT_FILLING;
      s.gen += 1;
      return &s;
    }
  }
  return nullptr;
}

void slot_set_state(nasr_ctx* h, BatchSlot* s, int st) {
  std::lock_guard<std::mutex> lk(h->slot_mu);
  s->state = st;
}

static bool stack_reshape(const nasr_ctx* h) {
  return h->lstm && h->lstm->cfg.merge == NASR_MERGE_STACK_RESHAPE && h->lstm->D == 2;
}

// slot_fill (1): the argument checks, in this order; *masked: aug has a mask of non-zero width
static int check_batch(nasr_ctx* h, const BatchSrc& b, bool* masked) {
  *masked = false;
  if ((b.feats != nullptr) + (b.centre != nullptr) + (b.producer != nullptr) + (b.stacked != nullptr) != 1 || !b.seq_len)
    return h->fail(NASR_ERR_ARG, "null input buffer");
  if (b.centre_form() && ((b.centre && !b.pad_value) || b.ctx < 0 || b.ncep < 1 || (2 * b.ctx + 1) * b.ncep != h->F))
    return h->fail(NASR_ERR_ARG, "context upload: feature_size must equal (2*numcontext+1)*numcep");
  if (b.labels && !b.label_len) return h->fail(NASR_ERR_ARG, "labels without label_len");
  if (b.chunk) return validate_chunk(h, b.seq_len, b.B, b.T);
  if (int rc = validate_batch(h, b.seq_len, b.labels, b.label_len, b.B, b.T, b.Lmax, 0, lstm_frame_skip(h))) return rc;
  if (!b.aug) return NASR_OK;
  if (!b.centre_form()) return h->fail(NASR_ERR_ARG, "augmentation masks need a batch in the centre form");
  return validate_aug(h, b.aug, b.seq_len, b.B, b.ctx, b.ncep, masked);
}

// slot_fill (2): the slot's shape and the layout of its meta block (int32): seq [Bp] | seqin [Bp] | lablen [Bp] |
// labels [B*Lm] | cstart [B*(C+1)] | cpos [B*Lm] | rowmap [Tp*Bp] | vrow, vprev, vnext [Rvp] | masks [B*nm] of int4.  seq:
// the lengths in the frames the network sees, seqin: the caller's (the same without a frame skip).  T below is the network's
// frame count: the caller's input T only sizes dfeats.  No HIP call.
static void meta_layout(nasr_ctx* h, BatchSlot* s, const BatchSrc& b, bool masked) {
  const LstmState* const ls = h->lstm.get();   // NULL: a handle of another family, which neither compacts rows nor runs windows
  s->skip = b.chunk ? 1 : lstm_frame_skip(h);  // (a stream chunk's rows are the kept ones already)
  const int B = b.B, T = skip_frames(b.T, s->skip);
  s->B = B; s->T = b.T; s->Tn = T; s->Lmax = b.labels ? b.Lmax : 0; s->ctx = b.ctx; s->ncep = b.ncep;
  s->Bp = rup(B, 16);
  s->Tp = ls ? lstm_logit_frames(h, T) : T;
  s->has_labels = b.labels != nullptr;
  s->centre = b.centre_form();
  s->masked = masked;
  s->aug_nm = masked ? std::max(b.aug->n_time, b.aug->n_freq) : 0;
  s->aug_sw = masked ? b.aug->static_width : 0;
  s->frames = s->nframes = 0;
  for (int i = 0; i < B; ++i) { s->frames += b.seq_len[i]; s->nframes += skip_frames(b.seq_len[i], s->skip); }
  const size_t BLm = (size_t)B * std::max(s->Lmax, 1);
  s->o_seq = 0;
  s->o_seqin = s->o_seq + s->Bp;
  s->o_lablen = s->o_seqin + s->Bp;
  s->o_labels = s->o_lablen + s->Bp;
  s->o_cstart = s->o_labels + BLm;
  s->o_cpos = s->o_cstart + (b.labels ? (size_t)B * (h->C + 1) : 0);
  s->o_rowmap = s->o_cpos + BLm;
  // compacted rows: worth it when at least 15 % of the T x Bp rows are padding (profiles/r03_row_compaction_ab.log: even at
  // 10 %), and only for training batches
  s->cmp = ls && ls->compactable && b.labels && s->nframes * 20 <= (int64_t)T * s->Bp * 17;
  s->Rv = s->cmp ? (int)s->nframes : 0;
  // a batch under nasr_set_chunking: the row lists are those of its windows, always (a stream chunk is no such batch)
  const bool lc = ls && ls->lcC > 0 && !b.chunk;
  s->chunk = b.chunk;
  s->lcC = lc ? ls->lcC : 0; s->lcR = lc ? ls->lcR : 0;
  s->lcW = lc ? std::min(s->lcC + s->lcR, T) : 0;      // (a window never has more rows than the batch has frames)
  s->lcK = lc ? lc_last_window(T, s->lcC, s->lcW) + 1 : 0;
  if (lc) {
    int64_t rows = 0;
    for (int i = 0; i < B; ++i)
      for (int k = 0; k < s->lcK; ++k) rows += lc_window_rows(skip_frames(b.seq_len[i], s->skip), k, s->lcC, s->lcW);
    s->cmp = true;
    s->Rv = (int)std::min<int64_t>(rows, (int64_t)1 << 22);   // (more: ensure_shape refuses the batch at commit)
  }
  s->Rvp = s->cmp ? rup(s->Rv, 64) : 0;
  s->o_vrow = s->o_rowmap + (stack_reshape(h) ? (size_t)s->Tp * s->Bp : 0);
  s->o_vprev = s->o_vrow + s->Rvp;
  s->o_vnext = s->o_vprev + s->Rvp;
  s->o_wlen = s->o_vnext + s->Rvp;
  const size_t end = s->o_wlen + (size_t)s->lcK * s->Bp;
  s->o_aug = (end + 3) / 4 * 4;      // (the kernel reads a mask as one int4)
  s->nmeta = masked ? s->o_aug + (size_t)B * s->aug_nm * 4 : end;
  s->nfeat = s->centre ? (size_t)B * b.T * b.ncep + B : (size_t)B * b.T * h->F;   // (the caller's frames, all of them)
}

// slot_fill (3): the meta block, as laid out, into the slot's pinned mirror
static void write_meta(const nasr_ctx* h, BatchSlot* s, const BatchSrc& src) {
  const int B = src.B, T = s->Tn, Bp = s->Bp, Tp = s->Tp, C = h->C, Lmax = src.Lmax, Lm = std::max(s->Lmax, 1), nm = s->aug_nm;
  const int32_t *labels = src.labels, *label_len = src.label_len;
  const nasr_batch_aug* aug = src.aug;
  int32_t* m = static_cast<int32_t*>(s->hmeta.get());
  memset(m, 0, s->nmeta * 4);
  memcpy(m + s->o_seqin, src.seq_len, (size_t)B * 4);
  for (int b = 0; b < B; ++b) m[s->o_seq + b] = skip_frames(src.seq_len[b], s->skip);
  const int32_t* seq_len = m + s->o_seq;   // from here on: frames the network sees
  if (labels) {
    memcpy(m + s->o_lablen, label_len, (size_t)B * 4);
    if (Lmax > 0) memcpy(m + s->o_labels, labels, (size_t)B * Lmax * 4);
    // the label positions of every utterance sorted by class (counting sort): the fixed summation order of ctc_grad
    std::vector<int32_t> fill;
    for (int b = 0; b < B; ++b)
      ctc_class_positions(labels + (size_t)b * Lmax, label_len[b], C, m + s->o_cstart + (size_t)b * (C + 1),
                          m + s->o_cpos + (size_t)b * Lm, fill);
  }
  if (stack_reshape(h)) {
    // logits[t',b'] <- flat row q = b'*2T + t' of O = stack(fw,bw) [2,B,T,H];
    // physical row index in the [(t*Bp+b)*2 + d][Hp] view of the last layer's output.
    int32_t* map = m + s->o_rowmap;
    for (size_t i = 0; i < (size_t)Tp * Bp; ++i) map[i] = -1;
    for (int tp = 0; tp < Tp; ++tp)
      for (int bq = 0; bq < B; ++bq) {
        const int64_t q = (int64_t)bq * 2 * T + tp;
        const int d = (int)(q / ((int64_t)B * T));
        const int64_t rem = q % ((int64_t)B * T);
        const int b = (int)(rem / T), t = (int)(rem % T);
        map[(size_t)tp * Bp + bq] = (t * Bp + b) * 2 + d;
      }
  }
  if (s->lcC) {
    // The rows of the windows, window-major: vprev / vnext stay inside a window, except that the row before a window's
    // first one is the row its forward state was carried from, row C-1 of the window before (the h_{t-1} operand of the
    // recurrent weight gradient, as everywhere).
    const int Cc = s->lcC, W = s->lcW;
    int32_t *vr = m + s->o_vrow, *vp = m + s->o_vprev, *vn = m + s->o_vnext, *wl = m + s->o_wlen;
    int i = 0;
    for (int k = 0; k < s->lcK; ++k) {
      for (int b = 0; b < B; ++b) wl[(size_t)k * Bp + b] = lc_window_rows(seq_len[b], k, Cc, W);
      for (int tl = 0; tl < W && i < s->Rv; ++tl)
        for (int b = 0; b < B && i < s->Rv; ++b) {
          const int P = wl[(size_t)k * Bp + b];
          if (tl >= P) continue;
          const int r = (k * W + tl) * Bp + b;
          vr[i] = r;
          vp[i] = tl > 0 ? r - Bp : k > 0 ? ((k - 1) * W + Cc - 1) * Bp + b : -1;
          vn[i] = tl + 1 < P ? r + Bp : -1;
          ++i;
        }
    }
    for (; i < s->Rvp; ++i) vr[i] = vp[i] = vn[i] = -1;
  } else if (s->cmp) {
    int32_t *vr = m + s->o_vrow, *vp = m + s->o_vprev, *vn = m + s->o_vnext;
    int i = 0;
    for (int t = 0; t < T; ++t)
      for (int b = 0; b < B; ++b)
        if (seq_len[b] > t) {
          vr[i] = t * Bp + b;
          vp[i] = t > 0 ? (t - 1) * Bp + b : -1;
          vn[i] = t + 1 < seq_len[b] ? (t + 1) * Bp + b : -1;
          ++i;
        }
    for (; i < s->Rvp; ++i) vr[i] = vp[i] = vn[i] = -1;
  }
  if (s->masked)
    for (int b = 0; b < B; ++b)
      for (int k = 0; k < nm; ++k) {
        int32_t* q = m + s->o_aug + ((size_t)b * nm + k) * 4;
        if (k < aug->n_time) { q[0] = aug->time_mask[((size_t)b * aug->n_time + k) * 2]; q[1] = aug->time_mask[((size_t)b * aug->n_time + k) * 2 + 1]; }
        if (k < aug->n_freq) { q[2] = aug->freq_mask[((size_t)b * aug->n_freq + k) * 2]; q[3] = aug->freq_mask[((size_t)b * aug->n_freq + k) * 2 + 1]; }
      }
}

// slot_fill (4): the features into s->dfeats on stream cs.  `pinned_feats` false: hipMemcpyAsync from the caller's pageable
// memory, which returns when the source may be reused; true: through the slot's pinned feature buffer, a plain DMA that
// overlaps whatever the compute stream runs.  A producer's kernels write the centre frames and pad values (or, `stacked`,
// the stacked rows) themselves.
static int copy_feats(nasr_ctx* h, BatchSlot* s, const BatchSrc& b, hipStream_t cs, bool pinned_feats) {
  const size_t nc = s->nfeat - b.B;        // centre form: the centre frames, then one pad value per utterance
  float* d = s->dfeats.as<float>();
  if (b.producer || b.stacked) {
    const int rc = b.stacked ? b.stacked->run(d, cs) : b.producer->run(d, d + nc, pinned_feats ? s->hfeats.get() : nullptr, cs);
    // what the producer queued before it failed may still read the slot's pinned buffer: the next fill waits for it
    if (rc && hipEventRecord(s->ev_copy, cs) == hipSuccess) s->copy_valid = true;
    return rc;
  }
  if (pinned_feats) {
    float* p = static_cast<float*>(s->hfeats.get());
    memcpy(p, b.centre ? b.centre : b.feats, (b.centre ? nc : s->nfeat) * 4);
    if (b.centre) memcpy(p + nc, b.pad_value, (size_t)b.B * 4);
    HIPCHK(h, hipMemcpyAsync(d, p, s->nfeat * 4, hipMemcpyHostToDevice, cs));
  } else if (b.centre) {
    HIPCHK(h, hipMemcpyAsync(d, b.centre, nc * 4, hipMemcpyHostToDevice, cs));
    HIPCHK(h, hipMemcpyAsync(d + nc, b.pad_value, (size_t)b.B * 4, hipMemcpyHostToDevice, cs));
  } else {
    HIPCHK(h, hipMemcpyAsync(d, b.feats, s->nfeat * 4, hipMemcpyHostToDevice, cs));
  }
  return NASR_OK;
}

// Copies batch b into slot s, in the order the steps above are numbered: the integer arrays through the slot's pinned meta
// buffer, the features as copy_feats says.  A batch in the centre form differs from a stacked one only in what dfeats
// holds, and a produced one from a host one only in who writes it: the meta block and everything slot_commit does are the
// same.  aug: SpecAugment masks behind the rest of the meta block; without a mask of non-zero width the slot is what it
// is without aug.  All device copies (and a producer's kernels) go to stream cs and end with the slot's ev_copy.
static int slot_fill(nasr_ctx* h, BatchSlot* s, const BatchSrc& b, hipStream_t cs, bool pinned_feats) {
  bool masked = false;
  if (int rc = check_batch(h, b, &masked)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  meta_layout(h, s, b, masked);
  bool grew = false;
  if (!s->dmeta.ensure(s->nmeta * 4, &grew) || !s->dfeats.ensure(s->nfeat * 4, &grew) ||
      !pinned_ensure(s->hmeta, &s->hmeta_cap, s->nmeta * 4) ||
      (pinned_feats && !b.stacked &&
       !pinned_ensure(s->hfeats, &s->hfeats_cap, b.producer ? b.producer->stage_bytes : s->nfeat * 4)))
    return h->fail(NASR_ERR_HIP, "allocation of a batch slot failed");
  if (s->copy_valid) HIPCHK(h, hipEventSynchronize(s->ev_copy));          // the pinned mirrors are free to overwrite
  if (s->released_valid && cs != h->st) HIPCHK(h, hipStreamWaitEvent(cs, s->ev_released, 0));   // and the device side unread
  write_meta(h, s, b);
  if (int rc = copy_feats(h, s, b, cs, pinned_feats)) return rc;
  HIPCHK(h, hipMemcpyAsync(s->dmeta.p, s->hmeta, s->nmeta * 4, hipMemcpyHostToDevice, cs));
  HIPCHK(h, hipEventRecord(s->ev_copy, cs));
  s->copy_valid = true;
  return NASR_OK;
}

// Makes the filled slot the resident batch: the compute stream waits for its copies, the previous resident slot is
// released, and the features are laid out for the step (time-major rows, context windows, operand scales).
int slot_commit(nasr_ctx* h, BatchSlot* s) {
  LstmState* const ls = h->lstm.get();   // NULL: a handle of another family
  HIPCHK(h, hipSetDevice(h->device));
  // (a slot is laid out for the chunking of the moment it was filled; a stream chunk never is)
  if (ls && !s->chunk && (s->lcC != ls->lcC || s->lcR != (ls->lcC ? ls->lcR : 0)))
    return h->fail(NASR_ERR_STATE, "the batch was staged under another nasr_set_chunking than the handle has now: stage it again");
  if (ls && !s->chunk && s->skip != ls->skip)   // (and for the frame skip of that moment)
    return h->fail(NASR_ERR_STATE, "the batch was staged under another nasr_set_frame_skip (" + std::to_string(s->skip) +
                                       ") than the handle has now (" + std::to_string(ls->skip) + "): stage it again");
  int rc = ensure_shape(h, s->B, s->Tn, s->Lmax, s->lcC > 0);
  if (rc) return rc;
  const int B = s->B, T = s->T, Bp = h->Bp;   // T: the caller's input frames, as dfeats holds them
  {
    std::lock_guard<std::mutex> lk(h->slot_mu);
    if (h->cur && h->cur != s) {
      // every kernel that reads the old batch's arrays is already on the compute stream: an event here releases them
      (void)hipEventRecord(h->cur->ev_released, h->st);
      h->cur->released_valid = true;
      h->cur->state = SLOT_FREE;
    }
    s->state = SLOT_RESIDENT;
    h->cur = s;
  }
  HIPCHK(h, hipStreamWaitEvent(h->st, s->ev_copy, 0));
  int32_t* md = s->meta_d();
  const int32_t* seq_in = md + s->o_seqin;   // the input lengths: what the feature movers below decide on
  // seq_len lives at a FIXED address: the hipGraphs of the per-step recurrence captured it
  HIPCHK(h, hipMemcpyAsync(h->seqbuf.p, md + s->o_seq, (size_t)Bp * 4, hipMemcpyDeviceToDevice, h->st));
  h->seq_p = h->seqbuf.as<int32_t>(); h->lablen_p = md + s->o_lablen; h->labels_p = md + s->o_labels;
  h->cstart_p = md + s->o_cstart; h->cpos_p = md + s->o_cpos; h->rowmap_p = md + s->o_rowmap;
  // (staged with compaction on, switched off since: the slot's row lists go unused; s->cmp: only ever on an LSTM-family handle)
  const bool cmp = s->cmp && ls && (ls->compactable || s->lcC);
  h->wlen_p = md + s->o_wlen;
  h->cmp_rows = cmp ? s->Rv : 0;
  h->cmp_rows_p = cmp ? s->Rvp : 0;
  h->vrow_p = md + s->o_vrow; h->vprev_p = md + s->o_vprev; h->vnext_p = md + s->o_vnext;
  h->ev_used = 0;
  h->spans.clear();
  if (h->profiling) {
    (void)hipEventRecord(h->ev_total_a, h->st);
    h->window_open = true;
    h->total_valid = false;
  }
  h->h_seq.assign((size_t)Bp, 0);
  const int32_t* hm = static_cast<const int32_t*>(s->hmeta.get());
  for (int b = 0; b < B; ++b) h->h_seq[b] = hm[s->o_seq + b];
  h->frames = s->frames;
  h->Tin = T;
  {
    PhaseScope ps(h, PH_PACK);
    const bool lc = ls && ls->lc_live;
    float* x0 = (lc ? ls->lc_x0 : h->X0).as<float>();   // a chunked batch: the rows by frame first
    if (s->centre && s->masked)
      launch_expand_context_masked(s->dfeats.as<float>(), s->dfeats.as<float>() + (size_t)B * T * s->ncep, seq_in,
                                   md + s->o_aug, s->aug_nm, s->aug_sw, x0, B, Bp, T, s->ctx, s->ncep,
                                   h->Fp, h->st, s->skip);
    else if (s->centre)
      launch_expand_context(s->dfeats.as<float>(), s->dfeats.as<float>() + (size_t)B * T * s->ncep, seq_in,
                            x0, B, Bp, T, s->ctx, s->ncep, h->Fp, h->st, s->skip);
    else
      launch_pack_feats(s->dfeats.as<float>(), x0, B, Bp, T, h->F, h->Fp, h->st, s->skip, s->skip > 1 ? seq_in : nullptr);
    if (lc) launch_lc_gather(x0, h->wlen_p, h->X0.as<float>(), ls->lcg, h->Fp, h->st);   // ... and into the windows' rows
    if (ls)   // (the WaveNet's and LAS's GEMMs read the fp32 features as they are)
      pl_scales(h, h->X0.as<float>(), ls->Tv * Bp, h->Fp, h->Fp, &ls->sc_x0r, &ls->sc_x0c, h->st);
    if (h->cmp_rows)    // the feature rows' scales in the compacted order (layer 0's input GEMM)
      launch_gather_rows(ls->sc_cx.sp(), ls->sc_x0r.sp(), h->vrow_p, h->cmp_rows_p, 1.f, h->st),
      launch_gather_rows(ls->sc_cx.ip(), ls->sc_x0r.ip(), h->vrow_p, h->cmp_rows_p, 1.f, h->st);
    if (ls && s->has_labels && ls->npre == 0)   // layer-0 input with the frame index as contraction index, for dWx = X^T dG
      launch_tph_split2(h->X0.as<float>(), nullptr, ls->X0TTP.as<unsigned char>(), h->cmp_rows ? h->cmp_rows : ls->Tv * Bp, h->Fp, h->Fp,
                        nullptr, 1.f, ls->sc_x0c.sp(), 1.f, nullptr, h->st, h->cmp_rows ? h->vrow_p : nullptr);
    HIPCHK(h, hipGetLastError());
  }
  h->resident = true;
  h->have_grads = false;
  h->have_fwd = false;
  h->have_decoded = false;
  h->teach_valid = false;   // teacher logits belong to the batch they were given for
  return NASR_OK;
}

int upload(nasr_ctx* h, const BatchSrc& b) {
  BatchSlot* s = slot_acquire(h, false);
  if (!s) return h->fail(NASR_ERR_STATE, "every batch slot holds a staged batch: commit or discard one first");
  int rc = slot_fill(h, s, b, h->st, false);
  if (!rc) rc = slot_commit(h, s);
  if (rc && h->cur != s) slot_set_state(h, s, SLOT_FREE);
  return rc;
}

BatchSlot* slot_of_ticket(nasr_ctx* h, int ticket) {
  if (ticket < 0 || (ticket & 255) >= NSLOT) return nullptr;
  BatchSlot* s = &h->slots[ticket & 255];
  std::lock_guard<std::mutex> lk(h->slot_mu);
  return (s->state == SLOT_STAGED && (int)(s->gen & 0x7fffff) == (ticket >> 8)) ? s : nullptr;
}

int stage(nasr_ctx* h, const BatchSrc& b, int* ticket) {
  if (!ticket) return h->fail(NASR_ERR_ARG, "null ticket");
  *ticket = -1;
  BatchSlot* s = slot_acquire(h, true);
  if (!s) return h->fail(NASR_ERR_STATE, "no free batch slot: commit or discard a staged batch first");
  const int rc = slot_fill(h, s, b, h->cst, true);
  slot_set_state(h, s, rc ? SLOT_FREE : SLOT_STAGED);
  if (!rc) *ticket = (int)(s - h->slots) | (int)((s->gen & 0x7fffff) << 8);
  return rc;
}
}  // namespace nasr_impl
