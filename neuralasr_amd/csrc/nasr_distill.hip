// nasr_distill.hip — teacher-student distillation beside the CTC loss: the ABI calls that set the term,
// bring a teacher's logits to the student's resident batch and report the loss's two parts, and the term on host arrays
// (the kernels' direct test entry).  The term itself runs in the step: ctc_forward and logit_grads (nasr_pass.hip) over
// the kernels of ctc.hip (5).  Both CTC families answer; a LAS or featurizer handle does not.
#include "nasr_ctx.h"

using namespace nasr;
using namespace nasr_impl;

namespace {
// why handle h takes no part in distillation, or NULL: its logit rows must be frames of its utterances
const char* no_distill(const nasr_ctx* h) {
  if (h->family == Family::Las) return "a LAS handle has no CTC logit frames";
  if (h->family == Family::Lstm && lstm_logit_frames(h, 1) != 1)
    return "NASR_MERGE_STACK_RESHAPE: its logit rows mix frames of the whole padded batch, so no row is a frame to compare";
  return nullptr;
}

int teacher_buffers(nasr_ctx* h) {
  bool grew = false;
  if (!h->teach.ensure((size_t)h->Tp * h->Bp * h->Cp * 4, &grew) || !h->kd_parts.ensure(16, &grew))
    return h->fail(NASR_ERR_HIP, "hipMalloc of the teacher logits failed");
  return NASR_OK;
}
}  // namespace

extern "C" {

int nasr_set_distill(nasr_handle h, float weight, float temperature) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  const std::string fn = "nasr_set_distill";
  if (const char* why = no_distill(h)) return h->fail(NASR_ERR_STATE, fn + ": " + why);
  if (!std::isfinite(weight) || weight < 0.f || weight >= 1.f)
    return h->fail(NASR_ERR_ARG, fn + ": weight must be in [0, 1) (0 = off)");
  if (!std::isfinite(temperature) || temperature < 0.25f || temperature > 16.f)
    return h->fail(NASR_ERR_ARG, fn + ": temperature must be in [0.25, 16]");
  h->kd_weight = weight;
  h->kd_tau = temperature;
  return NASR_OK;
}

int nasr_get_distill(nasr_handle h, float* weight, float* temperature) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (weight) *weight = h->kd_weight;
  if (temperature) *temperature = h->kd_tau;
  return NASR_OK;
}

int nasr_set_teacher_logits(nasr_handle h, const float* logits) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  const std::string fn = "nasr_set_teacher_logits";
  if (const char* why = no_distill(h)) return h->fail(NASR_ERR_STATE, fn + ": " + why);
  if (!logits) return h->fail(NASR_ERR_ARG, fn + ": null logits");
  if (!h->resident) return h->fail(NASR_ERR_STATE, fn + ": no resident batch: teacher logits belong to one");
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = teacher_buffers(h)) return rc;
  const int Tp = h->Tp, B = h->B, Bp = h->Bp, C = h->C, Cp = h->Cp;
  std::vector<float> lg((size_t)Tp * Bp * Cp, 0.f);   // the kernels' layout: rows t*Bp + b of Cp floats
  for (int t = 0; t < Tp; ++t)
    for (int b = 0; b < B; ++b)
      memcpy(lg.data() + ((size_t)t * Bp + b) * Cp, logits + ((size_t)t * B + b) * C, (size_t)C * 4);
  // on the compute stream: behind every read of the buffer by the step before
  hipError_t e = hipMemcpyAsync(h->teach.p, lg.data(), lg.size() * 4, hipMemcpyHostToDevice, h->st);
  if (e == hipSuccess) e = hipMemsetAsync(h->kd_parts.as<float>() + 2, 0, 4, h->st);   // host logits carry no fault word
  const hipError_t es = hipStreamSynchronize(h->st);                                    // (the copy reads lg)
  HIPCHK(h, e);
  HIPCHK(h, es);
  h->teach_valid = true;
  return NASR_OK;
}

int nasr_take_teacher_logits(nasr_handle h, nasr_handle teacher) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  const std::string fn = "nasr_take_teacher_logits";
  if (!teacher) return h->fail(NASR_ERR_ARG, fn + ": null teacher handle");
  if (teacher == h) return h->fail(NASR_ERR_ARG, fn + ": a handle cannot be its own teacher");
  if (const char* why = no_distill(h)) return h->fail(NASR_ERR_STATE, fn + ": " + why);
  if (teacher->family == Family::Featurizer) return h->fail(NASR_ERR_STATE, fn + ": the teacher is a featurizer handle: it has no model");
  if (const char* why = no_distill(teacher)) return h->fail(NASR_ERR_STATE, fn + ": the teacher: " + why);
  if (teacher->device != h->device)
    return h->fail(NASR_ERR_STATE, fn + ": the teacher is on device " + std::to_string(teacher->device) + ", the student on device " +
                                       std::to_string(h->device));
  if (!h->resident) return h->fail(NASR_ERR_STATE, fn + ": no resident batch: teacher logits belong to one");
  if (!teacher->resident || !teacher->have_fwd)
    return h->fail(NASR_ERR_STATE, fn + ": the teacher has no completed forward pass on a resident batch of its own");
  auto differs = [&](const char* what, int mine, int theirs) {
    return h->fail(NASR_ERR_STATE, fn + ": " + what + " differs: student " + std::to_string(mine) + ", teacher " + std::to_string(theirs));
  };
  if (teacher->B != h->B) return differs("the batch size B", h->B, teacher->B);
  if (teacher->Tp != h->Tp) return differs("the number of logit frames", h->Tp, teacher->Tp);
  if (teacher->C != h->C) return differs("the number of classes C", h->C, teacher->C);
  for (int b = 0; b < h->B; ++b)
    if (teacher->h_seq[b] != h->h_seq[b])
      return differs(("seq_len[" + std::to_string(b) + "]").c_str(), h->h_seq[b], teacher->h_seq[b]);
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = teacher_buffers(h)) return rc;
  if (!h->ev_teach_ready) HIPCHK(h, hipEventCreateWithFlags(h->ev_teach_ready.out(), hipEventDisableTiming));
  if (!h->ev_teach_taken) HIPCHK(h, hipEventCreateWithFlags(h->ev_teach_taken.out(), hipEventDisableTiming));
  // The copy runs on the student's stream: behind every read of the buffer by the student's step before, and behind the
  // teacher's forward pass (first event).  The teacher's stream then waits for the copy (second event): its next forward
  // pass does not overwrite logits that are still being read.  No host synchronisation.
  HIPCHK(h, hipEventRecord(h->ev_teach_ready, teacher->st));
  HIPCHK(h, hipStreamWaitEvent(h->st, h->ev_teach_ready, 0));
  HIPCHK(h, hipMemcpyAsync(h->teach.p, teacher->logits.p, (size_t)h->Tp * h->Bp * h->Cp * 4, hipMemcpyDeviceToDevice, h->st));
  HIPCHK(h, hipMemcpyAsync(h->kd_parts.as<float>() + 2, teacher->Gbase, 4, hipMemcpyDeviceToDevice, h->st));   // its fault word
  HIPCHK(h, hipEventRecord(h->ev_teach_taken, h->st));
  HIPCHK(h, hipStreamWaitEvent(teacher->st, h->ev_teach_taken, 0));
  h->teach_valid = true;
  return NASR_OK;
}

int nasr_get_distill_loss(nasr_handle h, float* ctc, float* kd) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (h->family == Family::Las) return h->fail(NASR_ERR_STATE, "nasr_get_distill_loss: a LAS handle has no CTC loss");
  if (!h->loss.p) return h->fail(NASR_ERR_STATE, "nasr_get_distill_loss: no loss pass has run");
  float parts[2] = {0.f, 0.f};
  if (h->kd_live)
    HIPCHK(h, hipMemcpyAsync(parts, h->kd_parts.p, 8, hipMemcpyDeviceToHost, h->st));
  else
    HIPCHK(h, hipMemcpyAsync(parts, h->loss.p, 4, hipMemcpyDeviceToHost, h->st));   // the plain loss; kd = 0
  if (int rc = sync_checked(h)) return rc;
  if (ctc) *ctc = parts[0];
  if (kd) *kd = parts[1];
  return NASR_OK;
}

int nasr_distill_logits(nasr_handle h, const float* student, const float* teacher, const int32_t* seq_len, int B, int Tp,
                        float weight, float temperature, float* dlogits_out, double* kd_out) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  const std::string fn = "nasr_distill_logits";
  if (h->family == Family::Las) return h->fail(NASR_ERR_STATE, fn + ": a LAS handle has no CTC logit frames");
  if (!student || !teacher || !seq_len || !dlogits_out || !kd_out) return h->fail(NASR_ERR_ARG, fn + ": null buffer");
  if (B < 1 || Tp < 1) return h->fail(NASR_ERR_ARG, fn + ": B and Tp must be >= 1");
  if (!std::isfinite(weight) || weight < 0.f || weight >= 1.f) return h->fail(NASR_ERR_ARG, fn + ": weight must be in [0, 1)");
  if (!std::isfinite(temperature) || temperature < 0.25f || temperature > 16.f)
    return h->fail(NASR_ERR_ARG, fn + ": temperature must be in [0.25, 16]");
  for (int b = 0; b < B; ++b)
    if (seq_len[b] < 1 || seq_len[b] > Tp)
      return h->fail(NASR_ERR_ARG, fn + ": seq_len[" + std::to_string(b) + "] = " + std::to_string(seq_len[b]) + " outside [1, Tp]");
  const int C = h->C, Cp = h->Cp, Bp = rup(B, 16);
  if ((size_t)Tp * Bp * Cp * 4 >= ((size_t)1 << 32)) return h->fail(NASR_ERR_ARG, fn + ": T' x B x C logits beyond 32-bit offsets");
  HIPCHK(h, hipSetDevice(h->device));
  // buffers of the call's own: the handle's state, the resident batch and its teacher logits stay as they were
  const size_t n = (size_t)Tp * Bp * Cp;
  DevBuf zs, ys, dg, kr, ks, sq;
  bool grew = false;
  if (!zs.ensure(n * 4, &grew) || !ys.ensure(n * 4, &grew) || !dg.ensure(n * 4, &grew) || !kr.ensure((size_t)Tp * Bp * 4, &grew) ||
      !ks.ensure((size_t)Bp * 8, &grew) || !sq.ensure((size_t)Bp * 4, &grew))
    return h->fail(NASR_ERR_HIP, fn + ": hipMalloc of the workspaces failed");
  std::vector<float> hz(n, 0.f), hy(n, 0.f), hd(n);
  for (int t = 0; t < Tp; ++t)
    for (int b = 0; b < B; ++b) {
      memcpy(hz.data() + ((size_t)t * Bp + b) * Cp, student + ((size_t)t * B + b) * C, (size_t)C * 4);
      memcpy(hy.data() + ((size_t)t * Bp + b) * Cp, teacher + ((size_t)t * B + b) * C, (size_t)C * 4);
    }
  std::vector<int32_t> hs((size_t)Bp, 0);
  std::copy(seq_len, seq_len + B, hs.begin());
  std::vector<double> hk((size_t)B);
  CtcDims d;
  d.Tp = Tp; d.B = B; d.Bp = Bp; d.C = C; d.Cp = Cp; d.Lmax = 1; d.KS = 0; d.Tws = 0;
  // from the first copy on every way out passes a stream synchronise: the copies read and write the vectors above
  auto run = [&]() -> int {
    HIPCHK(h, hipMemcpyAsync(zs.p, hz.data(), n * 4, hipMemcpyHostToDevice, h->st));
    HIPCHK(h, hipMemcpyAsync(ys.p, hy.data(), n * 4, hipMemcpyHostToDevice, h->st));
    HIPCHK(h, hipMemcpyAsync(sq.p, hs.data(), (size_t)Bp * 4, hipMemcpyHostToDevice, h->st));
    launch_distill_rows(d, zs.as<float>(), ys.as<float>(), sq.as<int>(), weight, temperature, dg.as<float>(), kr.as<float>(),
                        ks.as<double>(), h->st);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(hd.data(), dg.p, n * 4, hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipMemcpyAsync(hk.data(), ks.p, (size_t)B * 8, hipMemcpyDeviceToHost, h->st));
    return sync_checked(h);
  };
  const int rc = run();
  if (rc) {
    (void)hipStreamSynchronize(h->st);
    return rc;
  }
  for (int t = 0; t < Tp; ++t)
    for (int b = 0; b < B; ++b)
      memcpy(dlogits_out + ((size_t)t * B + b) * C, hd.data() + ((size_t)t * Bp + b) * Cp, (size_t)C * 4);
  std::copy(hk.begin(), hk.end(), kd_out);
  return NASR_OK;
}

}  // extern "C"
