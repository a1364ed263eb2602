// nasr_rec.hip — the recurrence's kind (nasr_ctx.h): create-time set-up and census of the resident kind, its launches,
// the abort check and re-arming, the recurrent-weight images of repack(), nasr_get/set_recurrence_mode.  See DESIGN.md §4.
#include "nasr_lstm.h"

namespace nasr_impl {

// Census: two steps of both persistent kernels on a zero layer.  A chip that does not place 32 workgroups on each of
// its 8 XCDs (partition modes, masked CUs, a co-tenant) is detected here and served by the per-step kernels.
// Synchronises the stream.
static bool persist_census(nasr_ctx* h) {
  LstmState* const ls = h->lstm.get();
  const int Bp = 16, T = 2;
  const size_t R = (size_t)T * Bp;
  DevBuf g, c, o, dg, sq;
  bool grew = false;
  bool ok = g.ensure(R * ls->D * ls->N4 * 4, &grew) && c.ensure(R * ls->D * ls->Hp * 4, &grew) &&
            o.ensure(R * ls->D * ls->Hp * 4, &grew) && dg.ensure(R * ls->D * ls->N4 * 4, &grew) && sq.ensure(Bp * 4, &grew);
  if (ok) {
    (void)hipMemsetAsync(g.p, 0, R * ls->D * ls->N4 * 4, h->st);
    (void)hipMemsetAsync(o.p, 0, R * ls->D * ls->Hp * 4, h->st);
    std::vector<int32_t> two((size_t)Bp, T);
    (void)hipMemcpyAsync(sq.p, two.data(), Bp * 4, hipMemcpyHostToDevice, h->st);
    const LstmDims dm{T, Bp, Bp, ls->H, ls->Hp, ls->D};
    launch_lstm_persist_fwd(dm, ls->Upf, ls->rec_f16 ? ls->Ucinv : nullptr, g.as<float>(), c.as<float>(), o.as<float>(),
                            sq.as<int>(), ls->xchf, ls->pctl, ls->perr, nullptr, 1.f, h->st);
    launch_lstm_persist_bwd(dm, ls->Upb, g.as<float>(), dg.as<float>(), c.as<float>(), o.as<float>(), sq.as<int>(),
                            ls->xchb, ls->pctl, ls->perr, nullptr, h->st, false, nullptr, nullptr, ls->bwd_lean);
    ok = hipStreamSynchronize(h->st) == hipSuccess && hipGetLastError() == hipSuccess && *ls->perr == 0;
  }
  *ls->perr = 0;
  return ok;
}

int rec_setup(nasr_ctx* h, bool allowed, bool f32) {
  LstmState* const ls = h->lstm.get();
  ls->rec_kind = !allowed ? RecKind::Step : persist_supported(ls->Hp) ? RecKind::Persist
                : wide_supported(ls->Hp, 16) ? RecKind::Wide : RecKind::Step;
  if (ls->rec_kind == RecKind::Step) return NASR_OK;
  ls->rec_f16 = ls->rec_kind == RecKind::Persist && !f32;
  const size_t nk = (size_t)ls->L * ls->D;
  bool g2 = false;   // the column scales: the wide images, the fp16 planes of the persistent kind
  if (hipHostMalloc(ls->perr.out(), 64, hipHostMallocMapped) != hipSuccess || hipMalloc(ls->Ucs.out(), nk * ls->N4 * 4) != hipSuccess ||
      hipMalloc(ls->Ucinv.out(), nk * ls->N4 * 4) != hipSuccess || !ls->scws.ensure(nk * tph_scale_ws_floats(ls->Hp, ls->N4) * 4, &g2))
    return h->fail(NASR_ERR_HIP, "allocation of the recurrent-weight scales failed");
  *ls->perr = 0;
  if (ls->rec_f16) {   // the census reads Ucinv before the first repack
    (void)hipMemsetAsync(ls->Ucs, 0, nk * ls->N4 * 4, h->st);
    (void)hipMemsetAsync(ls->Ucinv, 0, nk * ls->N4 * 4, h->st);
  }
  if (ls->rec_kind == RecKind::Persist) {
    ls->imf = persist_image_floats(ls->Hp, false);
    ls->imb = persist_image_floats(ls->Hp, true);
    if (persist_prepare() != hipSuccess || hipMalloc(ls->Upf.out(), nk * ls->imf * 4) != hipSuccess ||
        hipMalloc(ls->Upb.out(), nk * ls->imb * 4) != hipSuccess ||
        hipMalloc(ls->xchf.out(), (size_t)ls->L * persist_hx_bytes(ls->Hp)) != hipSuccess ||
        hipMalloc(ls->xchb.out(), (size_t)ls->L * persist_px_bytes()) != hipSuccess ||
        hipMalloc(ls->pctl.out(), (size_t)(1 + 2 * ls->L) * sizeof(PersistCtl)) != hipSuccess)   // [0] census, then one per layer pass
      return h->fail(NASR_ERR_HIP, "allocation of the persistent-recurrence buffers failed");
    (void)hipMemsetAsync(ls->Upf, 0, nk * ls->imf * 4, h->st);
    (void)hipMemsetAsync(ls->Upb, 0, nk * ls->imb * 4, h->st);
    return NASR_OK;
  }
  if (wide_prepare() != hipSuccess || hipMalloc(ls->Uw.out(), nk * wide_image_bytes(ls->Hp)) != hipSuccess ||
      hipMalloc(ls->whx.out(), wide_hx_bytes(64)) != hipSuccess || hipMalloc(ls->wpart.out(), wide_part_bytes(64)) != hipSuccess ||
      hipMalloc(ls->wctl.out(), sizeof(WideCtl)) != hipSuccess || hipMalloc(ls->Uwb.out(), nk * wide_image_bytes(ls->Hp)) != hipSuccess ||
      hipMalloc(ls->wpx.out(), wide_px_bytes(64)) != hipSuccess || hipMalloc(ls->Urs.out(), nk * ls->Hp * 4) != hipSuccess ||
      hipMalloc(ls->Urinv.out(), nk * ls->Hp * 4) != hipSuccess || hipMalloc(ls->wsrow.out(), 2 * 64 * 4) != hipSuccess)
    return h->fail(NASR_ERR_HIP, "allocation of the wide persistent-recurrence buffers failed");
  (void)hipMemsetAsync(ls->whx, 0, wide_hx_bytes(64), h->st);
  (void)hipMemsetAsync(ls->wpx, 0, wide_px_bytes(64), h->st);
  return NASR_OK;
}

void rec_start(nasr_ctx* h) {
  LstmState* const ls = h->lstm.get();
  if (ls->rec_kind == RecKind::Persist && !persist_census(h)) ls->rec_kind = RecKind::Step;   // its buffers stay
  ls->rec_use = ls->rec_kind;
  ls->rec_wanted = ls->rec_kind != RecKind::Step;
}

// a whole layer pass with a resident kind in use (run_steps); *launches += the recurrence launches enqueued
int rec_launch(nasr_ctx* h, int l, bool bwd, hipStream_t st, int* launches) {
  LstmState* const ls = h->lstm.get();
  const LstmDims dm{h->T, h->B, h->Bp, ls->H, ls->Hp, ls->D};
  if (ls->rec_use == RecKind::Persist) {
    const size_t k = (size_t)l * ls->D;
    if (!bwd) {
      launch_lstm_persist_fwd(dm, ls->Upf + k * ls->imf, ls->rec_f16 ? ls->Ucinv + k * ls->N4 : nullptr,
                              ls->gates[l].as<float>(), ls->cbuf[l].as<float>(),
                              ls->outb[l].as<float>(), h->seq_p, ls->xchf + (size_t)l * (persist_hx_bytes(ls->Hp) / 4),
                              ls->pctl + 1 + l, ls->perr, h->Gbase, ls->cfg.forget_bias, st, true);
    } else {
      launch_lstm_persist_bwd(dm, ls->Upb + k * ls->imb, ls->gates[l].as<float>(), dg_of(ls, l), ls->cbuf[l].as<float>(),
                              dout_of(ls, l), h->seq_p, ls->xchb + (size_t)l * (persist_px_bytes() / 4), ls->pctl + 1 + ls->L + l,
                              ls->perr, h->Gbase, st, true, ls->dgmax.as<float>(),
                              ls->dgmax.as<float>() + (size_t)ls->D * 32 * h->T * h->Bp, ls->bwd_lean);
      ls->dgmax_layer = l;
    }
    *launches += 1;
  } else {
    // the wide kind takes every batch: Bp = rup(B, 16) with B in [1, 64] (nasr_batch.hip's limit), the Bp of wide_supported
    if (bwd) launch_wide_row_scales(dm, dout_of(ls, l), h->seq_p, ls->wsrow, st);
    for (int d = 0; d < ls->D; ++d) {
      const size_t k = (size_t)l * ls->D + d;
      if (!bwd)
        launch_lstm_wide_fwd(dm, d, ls->Uw + k * wide_image_bytes(ls->Hp), ls->Ucinv + k * ls->N4, ls->gates[l].as<float>(),
                             ls->cbuf[l].as<float>(), ls->outb[l].as<float>(), h->seq_p, ls->whx, ls->wpart, ls->wctl, ls->perr,
                             h->Gbase, ls->cfg.forget_bias, st);
      else
        launch_lstm_wide_bwd(dm, d, ls->Uwb + k * wide_image_bytes(ls->Hp), ls->Urinv + k * ls->Hp, ls->wsrow,
                             ls->gates[l].as<float>(), dg_of(ls, l), ls->cbuf[l].as<float>(), dout_of(ls, l), h->seq_p, ls->wpart,
                             ls->wpx, ls->wctl, ls->perr, h->Gbase, st);
    }
    *launches += ls->D;
  }
  ls->rec_inflight = true;
  HIPCHK(h, hipGetLastError());
  return NASR_OK;
}

int rec_check(nasr_ctx* h) {
  LstmState* const ls = h->lstm.get();
  if (!ls || !ls->rec_inflight) return NASR_OK;
  ls->rec_inflight = false;
  const unsigned code = *reinterpret_cast<volatile unsigned*>(ls->perr.get());
  if (!code) return NASR_OK;
  *reinterpret_cast<volatile unsigned*>(ls->perr.get()) = 0;
  ls->rec_use = RecKind::Step;
  ls->rec_refused = true;
  ls->persist_aborts += 1;
  ls->clean_steps = 0;
  ls->rearm_wait = ls->persist_aborts <= 1 ? ls->rearm_after : std::min<int64_t>(ls->rearm_wait * 2, (int64_t)1 << 20);
  (void)repack(h);   // operand images of the per-step kernels
  return h->fail(NASR_ERR_HIP, "persistent recurrence aborted (code " + std::to_string(code) +
                                   ": 1 = hand-off timeout, 2 = workgroup placement, 4 = dG beyond its fp16 planes); the results of this step are "
                                   "invalid, later steps use the per-step kernels" +
                                   (ls->rearm_wait > 0 ? " (the persistent kernels are tried again after " +
                                                            std::to_string(ls->rearm_wait) + " clean steps)"
                                                      : ""));
}

// After `rearm_wait` clean steps on the per-step kernels: back to the kind (called at the start of a step, before
// anything of it is enqueued).  The persistent kind runs the census again first; the wide kind's next launch is its
// census (a second abort voids that step, which the caller repeats on the per-step kernels, and doubles the wait).
void rec_rearm(nasr_ctx* h) {
  LstmState* const ls = h->lstm.get();
  if (!ls || ls->rec_use != RecKind::Step || !ls->rec_wanted || ls->persist_aborts == 0 || ls->rearm_wait <= 0) return;
  if (++ls->clean_steps <= ls->rearm_wait) return;   // `rearm_wait` whole steps ran on the per-step kernels since the abort
  ls->clean_steps = 0;
  if (hipStreamSynchronize(h->st) != hipSuccess) return;
  // the operand images of the kind are stale (repack() only maintains the kind in use): rebuild first
  ls->rec_use = ls->rec_kind;
  if (repack(h) != NASR_OK || (ls->rec_kind == RecKind::Persist && !persist_census(h))) {
    ls->rec_use = RecKind::Step;
    ls->rearm_wait = std::min<int64_t>(ls->rearm_wait * 2, (int64_t)1 << 20);
    (void)repack(h);
    return;
  }
  ls->rec_refused = false;
  ls->persist_rearms += 1;
  drop_graphs(h);
}

std::vector<TphScaleJob> rec_scale_jobs(const nasr_ctx* h) {
  const LstmState* const ls = h->lstm.get();
  std::vector<TphScaleJob> jobs;
  for (size_t k = 0; k < ls->off_u.size(); ++k) {
    const float* U = h->P + ls->off_u[k];
    if (ls->rec_use == RecKind::Persist && ls->rec_f16)
      jobs.push_back({U, ls->Hp, ls->N4, ls->N4, nullptr, nullptr, ls->Ucs + k * ls->N4, ls->Ucinv + k * ls->N4});
    else if (ls->rec_use == RecKind::Wide)
      jobs.push_back({U, ls->Hp, ls->N4, ls->N4, ls->Urs + k * ls->Hp, ls->Urinv + k * ls->Hp, ls->Ucs + k * ls->N4, ls->Ucinv + k * ls->N4});
  }
  return jobs;
}

// the per-step kernels' images of every recurrent matrix, from the parameters as they are
static void step_images(nasr_ctx* h) {
  LstmState* const ls = h->lstm.get();
  for (size_t k = 0; k < ls->off_u.size(); ++k)
    launch_repack_u(h->P + ls->off_u[k], ls->Uf + k * ls->Hp * ls->N4, ls->Ub + k * ls->Hp * ls->N4, ls->Hp, h->st);
  ls->step_img_seq = ls->repack_seq;
}

void rec_images(nasr_ctx* h) {
  LstmState* const ls = h->lstm.get();
  if (ls->rec_use == RecKind::Persist) {
    launch_repack_persist(h->P, ls->off_u.data(), (int)ls->off_u.size(), ls->Upf, ls->Upb, ls->Hp, ls->rec_f16 ? ls->Ucs : nullptr, h->st);
  } else if (ls->rec_use == RecKind::Wide) {   // fp16-plane images under the scales of rec_scale_jobs
    for (size_t k = 0; k < ls->off_u.size(); ++k) {
      const float* U = h->P + ls->off_u[k];
      launch_repack_wide(U, ls->Ucs + k * ls->N4, ls->Uw + k * wide_image_bytes(ls->Hp), ls->Hp, h->st);
      launch_repack_wide_bwd(U, ls->Urs + k * ls->Hp, ls->Uwb + k * wide_image_bytes(ls->Hp), ls->Hp, h->st);
    }
  } else {
    step_images(h);
  }
}

void ensure_step_images(nasr_ctx* h) {
  LstmState* const ls = h->lstm.get();
  if (ls->rec_use != RecKind::Step && ls->step_img_seq != ls->repack_seq) step_images(h);
}

}  // namespace nasr_impl

extern "C" int nasr_get_recurrence_mode(nasr_handle h) {
  MODEL_CALL(h);
  LSTM_CALL(h, "has no recurrence");
  return h ? (int)h->lstm->rec_use : 0;
}

extern "C" int nasr_set_recurrence_mode(nasr_handle h, int persistent) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  LSTM_CALL(h, "has no recurrence");
  LstmState* const ls = h->lstm.get();
  if (persistent && ls->rec_kind != RecKind::Wide && (ls->rec_kind == RecKind::Step || ls->rec_refused))
    return h->fail(NASR_ERR_STATE, "the persistent recurrence is not available on this device / hidden size");
  HIPCHK(h, hipStreamSynchronize(h->st));
  ls->rec_use = persistent ? ls->rec_kind : RecKind::Step;
  ls->rec_wanted = persistent != 0;
  return repack(h);
}
