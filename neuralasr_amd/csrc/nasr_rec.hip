// nasr_rec.hip — the recurrence's kind (nasr_ctx.h): create-time set-up and census of the resident kind, its launches,
// the abort check and re-arming, the recurrent-weight images of repack(), nasr_get/set_recurrence_mode.  See DESIGN.md §4.
#include "nasr_ctx.h"

namespace nasr_impl {

// Census: two steps of both persistent kernels on a zero layer.  A chip that does not place 32 workgroups on each of
// its 8 XCDs (partition modes, masked CUs, a co-tenant) is detected here and served by the per-step kernels.
// Synchronises the stream.
static bool persist_census(nasr_ctx* h) {
  const int Bp = 16, T = 2;
  const size_t R = (size_t)T * Bp;
  DevBuf g, c, o, dg, sq;
  bool grew = false;
  bool ok = g.ensure(R * h->D * h->N4 * 4, &grew) && c.ensure(R * h->D * h->Hp * 4, &grew) &&
            o.ensure(R * h->D * h->Hp * 4, &grew) && dg.ensure(R * h->D * h->N4 * 4, &grew) && sq.ensure(Bp * 4, &grew);
  if (ok) {
    (void)hipMemsetAsync(g.p, 0, R * h->D * h->N4 * 4, h->st);
    (void)hipMemsetAsync(o.p, 0, R * h->D * h->Hp * 4, h->st);
    std::vector<int32_t> two((size_t)Bp, T);
    (void)hipMemcpyAsync(sq.p, two.data(), Bp * 4, hipMemcpyHostToDevice, h->st);
    const LstmDims dm{T, Bp, Bp, h->H, h->Hp, h->D};
    launch_lstm_persist_fwd(dm, h->Upf, h->rec_f16 ? h->Ucinv : nullptr, g.as<float>(), c.as<float>(), o.as<float>(),
                            sq.as<int>(), h->xchf, h->pctl, h->perr, nullptr, 1.f, h->st);
    launch_lstm_persist_bwd(dm, h->Upb, g.as<float>(), dg.as<float>(), c.as<float>(), o.as<float>(), sq.as<int>(),
                            h->xchb, h->pctl, h->perr, nullptr, h->st, false, nullptr, nullptr, h->bwd_lean);
    ok = hipStreamSynchronize(h->st) == hipSuccess && hipGetLastError() == hipSuccess && *h->perr == 0;
  }
  *h->perr = 0;
  return ok;
}

int rec_setup(nasr_ctx* h, bool allowed, bool f32) {
  h->rec_kind = !allowed ? RecKind::Step : persist_supported(h->Hp) ? RecKind::Persist
                : wide_supported(h->Hp, 16) ? RecKind::Wide : RecKind::Step;
  if (h->rec_kind == RecKind::Step) return NASR_OK;
  h->rec_f16 = h->rec_kind == RecKind::Persist && !f32;
  const size_t nk = (size_t)h->L * h->D;
  bool g2 = false;   // the column scales: the wide images, the fp16 planes of the persistent kind
  if (hipHostMalloc(h->perr.out(), 64, hipHostMallocMapped) != hipSuccess || hipMalloc(h->Ucs.out(), nk * h->N4 * 4) != hipSuccess ||
      hipMalloc(h->Ucinv.out(), nk * h->N4 * 4) != hipSuccess || !h->scws.ensure(nk * tph_scale_ws_floats(h->Hp, h->N4) * 4, &g2))
    return h->fail(NASR_ERR_HIP, "allocation of the recurrent-weight scales failed");
  *h->perr = 0;
  if (h->rec_f16) {   // the census reads Ucinv before the first repack
    (void)hipMemsetAsync(h->Ucs, 0, nk * h->N4 * 4, h->st);
    (void)hipMemsetAsync(h->Ucinv, 0, nk * h->N4 * 4, h->st);
  }
  if (h->rec_kind == RecKind::Persist) {
    h->imf = persist_image_floats(h->Hp, false);
    h->imb = persist_image_floats(h->Hp, true);
    if (persist_prepare() != hipSuccess || hipMalloc(h->Upf.out(), nk * h->imf * 4) != hipSuccess ||
        hipMalloc(h->Upb.out(), nk * h->imb * 4) != hipSuccess ||
        hipMalloc(h->xchf.out(), (size_t)h->L * persist_hx_bytes(h->Hp)) != hipSuccess ||
        hipMalloc(h->xchb.out(), (size_t)h->L * persist_px_bytes()) != hipSuccess ||
        hipMalloc(h->pctl.out(), (size_t)(1 + 2 * h->L) * sizeof(PersistCtl)) != hipSuccess)   // [0] census, then one per layer pass
      return h->fail(NASR_ERR_HIP, "allocation of the persistent-recurrence buffers failed");
    (void)hipMemsetAsync(h->Upf, 0, nk * h->imf * 4, h->st);
    (void)hipMemsetAsync(h->Upb, 0, nk * h->imb * 4, h->st);
    return NASR_OK;
  }
  if (wide_prepare() != hipSuccess || hipMalloc(h->Uw.out(), nk * wide_image_bytes(h->Hp)) != hipSuccess ||
      hipMalloc(h->whx.out(), wide_hx_bytes(64)) != hipSuccess || hipMalloc(h->wpart.out(), wide_part_bytes(64)) != hipSuccess ||
      hipMalloc(h->wctl.out(), sizeof(WideCtl)) != hipSuccess || hipMalloc(h->Uwb.out(), nk * wide_image_bytes(h->Hp)) != hipSuccess ||
      hipMalloc(h->wpx.out(), wide_px_bytes(64)) != hipSuccess || hipMalloc(h->Urs.out(), nk * h->Hp * 4) != hipSuccess ||
      hipMalloc(h->Urinv.out(), nk * h->Hp * 4) != hipSuccess || hipMalloc(h->wsrow.out(), 2 * 64 * 4) != hipSuccess)
    return h->fail(NASR_ERR_HIP, "allocation of the wide persistent-recurrence buffers failed");
  (void)hipMemsetAsync(h->whx, 0, wide_hx_bytes(64), h->st);
  (void)hipMemsetAsync(h->wpx, 0, wide_px_bytes(64), h->st);
  return NASR_OK;
}

void rec_start(nasr_ctx* h) {
  if (h->rec_kind == RecKind::Persist && !persist_census(h)) h->rec_kind = RecKind::Step;   // its buffers stay
  h->rec_use = h->rec_kind;
  h->rec_wanted = h->rec_kind != RecKind::Step;
}

// a whole layer pass with a resident kind in use (run_steps); *launches += the recurrence launches enqueued
int rec_launch(nasr_ctx* h, int l, bool bwd, hipStream_t st, int* launches) {
  const LstmDims dm{h->T, h->B, h->Bp, h->H, h->Hp, h->D};
  if (h->rec_use == RecKind::Persist) {
    const size_t k = (size_t)l * h->D;
    if (!bwd) {
      launch_lstm_persist_fwd(dm, h->Upf + k * h->imf, h->rec_f16 ? h->Ucinv + k * h->N4 : nullptr,
                              h->gates[l].as<float>(), h->cbuf[l].as<float>(),
                              h->outb[l].as<float>(), h->seq_p, h->xchf + (size_t)l * (persist_hx_bytes(h->Hp) / 4),
                              h->pctl + 1 + l, h->perr, h->Gbase, h->cfg.forget_bias, st, true);
    } else {
      launch_lstm_persist_bwd(dm, h->Upb + k * h->imb, h->gates[l].as<float>(), dg_of(h, l), h->cbuf[l].as<float>(),
                              dout_of(h, l), h->seq_p, h->xchb + (size_t)l * (persist_px_bytes() / 4), h->pctl + 1 + h->L + l,
                              h->perr, h->Gbase, st, true, h->dgmax.as<float>(),
                              h->dgmax.as<float>() + (size_t)h->D * 32 * h->T * h->Bp, h->bwd_lean);
      h->dgmax_layer = l;
    }
    *launches += 1;
  } else {
    // the wide kind takes every batch: Bp = rup(B, 16) with B in [1, 64] (nasr_batch.hip's limit), the Bp of wide_supported
    if (bwd) launch_wide_row_scales(dm, dout_of(h, l), h->seq_p, h->wsrow, st);
    for (int d = 0; d < h->D; ++d) {
      const size_t k = (size_t)l * h->D + d;
      if (!bwd)
        launch_lstm_wide_fwd(dm, d, h->Uw + k * wide_image_bytes(h->Hp), h->Ucinv + k * h->N4, h->gates[l].as<float>(),
                             h->cbuf[l].as<float>(), h->outb[l].as<float>(), h->seq_p, h->whx, h->wpart, h->wctl, h->perr,
                             h->Gbase, h->cfg.forget_bias, st);
      else
        launch_lstm_wide_bwd(dm, d, h->Uwb + k * wide_image_bytes(h->Hp), h->Urinv + k * h->Hp, h->wsrow,
                             h->gates[l].as<float>(), dg_of(h, l), h->cbuf[l].as<float>(), dout_of(h, l), h->seq_p, h->wpart,
                             h->wpx, h->wctl, h->perr, h->Gbase, st);
    }
    *launches += h->D;
  }
  h->rec_inflight = true;
  HIPCHK(h, hipGetLastError());
  return NASR_OK;
}

int rec_check(nasr_ctx* h) {
  if (!h->rec_inflight) return NASR_OK;
  h->rec_inflight = false;
  const unsigned code = *reinterpret_cast<volatile unsigned*>(h->perr.get());
  if (!code) return NASR_OK;
  *reinterpret_cast<volatile unsigned*>(h->perr.get()) = 0;
  h->rec_use = RecKind::Step;
  h->rec_refused = true;
  h->persist_aborts += 1;
  h->clean_steps = 0;
  h->rearm_wait = h->persist_aborts <= 1 ? h->rearm_after : std::min<int64_t>(h->rearm_wait * 2, (int64_t)1 << 20);
  (void)repack(h);   // operand images of the per-step kernels
  return h->fail(NASR_ERR_HIP, "persistent recurrence aborted (code " + std::to_string(code) +
                                   ": 1 = hand-off timeout, 2 = workgroup placement, 4 = dG beyond its fp16 planes); the results of this step are "
                                   "invalid, later steps use the per-step kernels" +
                                   (h->rearm_wait > 0 ? " (the persistent kernels are tried again after " +
                                                            std::to_string(h->rearm_wait) + " clean steps)"
                                                      : ""));
}

// After `rearm_wait` clean steps on the per-step kernels: back to the kind (called at the start of a step, before
// anything of it is enqueued).  The persistent kind runs the census again first; the wide kind's next launch is its
// census (a second abort voids that step, which the caller repeats on the per-step kernels, and doubles the wait).
void rec_rearm(nasr_ctx* h) {
  if (h->rec_use != RecKind::Step || !h->rec_wanted || h->persist_aborts == 0 || h->rearm_wait <= 0) return;
  if (++h->clean_steps <= h->rearm_wait) return;   // `rearm_wait` whole steps ran on the per-step kernels since the abort
  h->clean_steps = 0;
  if (hipStreamSynchronize(h->st) != hipSuccess) return;
  // the operand images of the kind are stale (repack() only maintains the kind in use): rebuild first
  h->rec_use = h->rec_kind;
  if (repack(h) != NASR_OK || (h->rec_kind == RecKind::Persist && !persist_census(h))) {
    h->rec_use = RecKind::Step;
    h->rearm_wait = std::min<int64_t>(h->rearm_wait * 2, (int64_t)1 << 20);
    (void)repack(h);
    return;
  }
  h->rec_refused = false;
  h->persist_rearms += 1;
  drop_graphs(h);
}

std::vector<TphScaleJob> rec_scale_jobs(const nasr_ctx* h) {
  std::vector<TphScaleJob> jobs;
  for (size_t k = 0; k < h->off_u.size(); ++k) {
    const float* U = h->P + h->off_u[k];
    if (h->rec_use == RecKind::Persist && h->rec_f16)
      jobs.push_back({U, h->Hp, h->N4, h->N4, nullptr, nullptr, h->Ucs + k * h->N4, h->Ucinv + k * h->N4});
    else if (h->rec_use == RecKind::Wide)
      jobs.push_back({U, h->Hp, h->N4, h->N4, h->Urs + k * h->Hp, h->Urinv + k * h->Hp, h->Ucs + k * h->N4, h->Ucinv + k * h->N4});
  }
  return jobs;
}

// the per-step kernels' images of every recurrent matrix, from the parameters as they are
static void step_images(nasr_ctx* h) {
  for (size_t k = 0; k < h->off_u.size(); ++k)
    launch_repack_u(h->P + h->off_u[k], h->Uf + k * h->Hp * h->N4, h->Ub + k * h->Hp * h->N4, h->Hp, h->st);
  h->step_img_seq = h->repack_seq;
}

void rec_images(nasr_ctx* h) {
  if (h->rec_use == RecKind::Persist) {
    launch_repack_persist(h->P, h->off_u.data(), (int)h->off_u.size(), h->Upf, h->Upb, h->Hp, h->rec_f16 ? h->Ucs : nullptr, h->st);
  } else if (h->rec_use == RecKind::Wide) {   // fp16-plane images under the scales of rec_scale_jobs
    for (size_t k = 0; k < h->off_u.size(); ++k) {
      const float* U = h->P + h->off_u[k];
      launch_repack_wide(U, h->Ucs + k * h->N4, h->Uw + k * wide_image_bytes(h->Hp), h->Hp, h->st);
      launch_repack_wide_bwd(U, h->Urs + k * h->Hp, h->Uwb + k * wide_image_bytes(h->Hp), h->Hp, h->st);
    }
  } else {
    step_images(h);
  }
}

void ensure_step_images(nasr_ctx* h) {
  if (h->rec_use != RecKind::Step && h->step_img_seq != h->repack_seq) step_images(h);
}

}  // namespace nasr_impl

extern "C" int nasr_get_recurrence_mode(nasr_handle h) {
  MODEL_CALL(h);
  LSTM_CALL(h, "has no recurrence");
  return h ? (int)h->rec_use : 0;
}

extern "C" int nasr_set_recurrence_mode(nasr_handle h, int persistent) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  LSTM_CALL(h, "has no recurrence");
  if (persistent && h->rec_kind != RecKind::Wide && (h->rec_kind == RecKind::Step || h->rec_refused))
    return h->fail(NASR_ERR_STATE, "the persistent recurrence is not available on this device / hidden size");
  HIPCHK(h, hipStreamSynchronize(h->st));
  h->rec_use = persistent ? h->rec_kind : RecKind::Step;
  h->rec_wanted = persistent != 0;
  return repack(h);
}
