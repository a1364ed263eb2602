// nasr_api.hip — the C ABI of include/nasr.h: every entry point names the reference interface it replaces there, and what
// the create calls of all handle kinds share (handle_open, alloc_param_buffers, handle_finish).  The work
// behind them lives in nasr_layout.hip (parameters, operand images), nasr_rec.hip (the recurrence, nasr_*_recurrence_mode),
// nasr_batch.hip (batches), nasr_pass.hip (the step) and nasr_comm.hip (RCCL); the shared handle is nasr_ctx.h.  Every call
// here serves every model family; the set-up of a handle and the calls that only one family answers stand in that family's
// file (nasr_lstm.hip, nasr_wavenet.hip, nasr_las.hip, nasr_fz.hip).  nasr_create is here for what it reads: the environment.
#include "nasr_ctx.h"

using namespace nasr;
using namespace nasr_impl;

namespace {
// the first check of a call that trains: while nasr_ema_swap has the average in P's place there is nothing to train
#define NOT_EMA_LIVE(h)                                                                                              \
  do {                                                                                                               \
    if ((h)->ema_live)                                                                                               \
      return (h)->fail(NASR_ERR_STATE, std::string(__func__) + ": the parameters hold their average (nasr_ema_swap); " \
                                                               "swap back first");                                   \
  } while (0)

int settle_end(nasr_ctx* h, nasr_ctx::StepEnd& e, int* void_out) {
  // the end of THAT step only
  if (!wait_stamp(e.stamp, e.seq, 60.0)) return h->fail(NASR_ERR_HIP, "nasr_settle_step: the step did not end within 60 s");
  if (*e.host != 0.f) {
    *void_out = 1;
    (void)rec_check(h);   // a local abort: this handle continues on the per-step kernels (message in last_error)
  }
  return NASR_OK;
}
}  // namespace

namespace nasr_impl {

int create_fail(nasr_ctx* h, int code, const std::string& m) {
  g_create_error = m;
  nasr_destroy(h);
  return code;
}

int handle_open(const char* fn, Family family, int device_id, void* stream, nasr_ctx** out, hipDeviceProp_t* prop) {
  auto refuse = [fn](int code, const std::string& m) {
    g_create_error = std::string(fn) + ": " + m;
    return code;
  };
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return refuse(NASR_ERR_HIP, "no HIP device visible (libnasr has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return refuse(NASR_ERR_ARG, "device_id out of range");
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, device_id) != hipSuccess) return refuse(NASR_ERR_HIP, "hipGetDeviceProperties failed");
  if (std::string(p.gcnArchName).find("gfx950") == std::string::npos)
    return refuse(NASR_ERR_HIP, std::string("device is ") + p.gcnArchName + ", libnasr is built for gfx950 only");
  if (prop) *prop = p;
  nasr_ctx* h = new nasr_ctx();
  h->family = family;
  h->device = device_id;
  if (hipSetDevice(device_id) != hipSuccess) return create_fail(h, NASR_ERR_HIP, "hipSetDevice failed");
  if (stream)
    h->st.borrow(reinterpret_cast<hipStream_t>(stream));
  else if (hipStreamCreateWithFlags(h->st.out(), hipStreamNonBlocking) != hipSuccess)
    return create_fail(h, NASR_ERR_HIP, "hipStreamCreate failed");
  *out = h;
  return NASR_OK;
}

bool alloc_param_buffers(nasr_ctx* h) {
  const size_t nb = (size_t)h->np_int * 4;
  const size_t gb = nb + GRAD_HEAD * 4;   // the gradient buffer starts with the fault word (+ padding): see nasr_grad_device_count
  if (hipMalloc(h->P.out(), nb) != hipSuccess || hipMalloc(h->M.out(), nb) != hipSuccess || hipMalloc(h->V.out(), nb) != hipSuccess ||
      hipMalloc(h->Gbase.out(), gb) != hipSuccess || hipMalloc(h->adam_dev.out(), sizeof(AdamDev)) != hipSuccess)
    return false;
  if (hipMalloc(h->clip_dev.out(), sizeof(ClipDev)) != hipSuccess ||
      hipMalloc(h->clip_part.out(), GRAD_SUMSQ_MAX_BLOCKS * sizeof(double)) != hipSuccess)
    return false;
  (void)hipMemsetAsync(h->adam_dev, 0, sizeof(AdamDev), h->st);
  static const ClipDev clip0{0.0, 1.f, 1.f, 0, 0, 0.0, 0, 0, 0};   // nothing measured yet: coef 1
  (void)hipMemcpyAsync(h->clip_dev, &clip0, sizeof(ClipDev), hipMemcpyHostToDevice, h->st);
  (void)hipMemsetAsync(h->clip_part, 0, GRAD_SUMSQ_MAX_BLOCKS * sizeof(double), h->st);
  (void)hipMemsetAsync(h->P, 0, nb, h->st);
  (void)hipMemsetAsync(h->M, 0, nb, h->st);
  (void)hipMemsetAsync(h->V, 0, nb, h->st);
  (void)hipMemsetAsync(h->Gbase, 0, gb, h->st);
  h->G = h->Gbase + GRAD_HEAD;
  return true;
}

int handle_finish(nasr_ctx* h) {
  h->ev_bucket.resize(h->buckets.size());
  for (Event& e : h->ev_bucket)
    if (hipEventCreateWithFlags(e.out(), hipEventDisableTiming) != hipSuccess) return create_fail(h, NASR_ERR_HIP, "hipEventCreate failed");
  if (hipStreamCreateWithFlags(h->cst.out(), hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(h->d2h.out(), hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(h->ev_snap.out(), hipEventDisableTiming) != hipSuccess)
    return create_fail(h, NASR_ERR_HIP, "hipStreamCreate failed");
  for (BatchSlot& bs : h->slots)
    if (hipEventCreateWithFlags(bs.ev_copy.out(), hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(bs.ev_released.out(), hipEventDisableTiming) != hipSuccess)
      return create_fail(h, NASR_ERR_HIP, "hipEventCreate failed");
  for (auto& r : h->res) {
    if (hipHostMalloc(r.stamp.out(), 64, hipHostMallocMapped) != hipSuccess)
      return create_fail(h, NASR_ERR_HIP, "set-up of the step-result stamps failed");
    *r.stamp = 0;
  }
  for (auto& e : h->endw) {
    if (hipHostMalloc(e.host.out(), 64, hipHostMallocMapped) != hipSuccess)
      return create_fail(h, NASR_ERR_HIP, "set-up of the step-end words failed");
    e.stamp = reinterpret_cast<uint32_t*>(e.host.get()) + 8;
    *e.host = 0.f;
    *e.stamp = 0;
  }
  (void)hipEventCreate(h->ev_total_a.out());
  (void)hipEventCreate(h->ev_total_b.out());
  memset(&h->last_times, 0, sizeof(h->last_times));
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(h->st) != hipSuccess)
    return create_fail(h, NASR_ERR_HIP, "stream synchronize failed in create");
  return NASR_OK;
}

}  // namespace nasr_impl

// =============================================================================== C ABI
extern "C" {

int nasr_create(const nasr_model_cfg* cfg, int device_id, void* stream, nasr_handle* out) {
  // the create-time switches of README: the environment is read here and nowhere else; the set-up takes them as values
  auto off = [](const char* name) { const char* e = getenv(name); return e && e[0] == '0'; };
  const char *rec = getenv("NASR_REC"), *rearm = getenv("NASR_PERSIST_REARM");
  LstmSwitches sw;
  sw.compact = !off("NASR_COMPACT");
  sw.persist = !off("NASR_PERSIST");
  sw.rec_f32 = rec && std::string(rec) == "f32";
  sw.wgrad_overlap = !off("NASR_WGRAD_OVERLAP");
  sw.bucket_defer = !off("NASR_BUCKET_DEFER");
  sw.rearm_after = rearm && *rearm ? std::max<long long>(0, atoll(rearm)) : 200;
  return lstm_create(cfg, device_id, stream, sw, out);
}

int nasr_destroy(nasr_handle h) {
  if (!h) return NASR_OK;
  (void)hipSetDevice(h->device);
  for (const Stream* s : {&h->st, &h->cst, &h->d2h})
    if (*s) (void)hipStreamSynchronize(*s);
  lstm_sync_side(h);
  (void)nasr_comm_destroy(h);
  drop_graphs(h);
  delete h;   // the owners in nasr_ctx release its memory, streams and events
  return NASR_OK;
}

const char* nasr_last_error(nasr_handle h) {
  if (!h) return g_create_error.c_str();
  return t_err_handle == h ? t_err.c_str() : "";
}
const char* nasr_backend(nasr_handle) { return "hip-gfx950"; }

int nasr_synchronize(nasr_handle h) {
  if (!h) return NASR_ERR_ARG;
  return sync_checked(h);
}

int64_t nasr_param_count(nasr_handle h) {
  MODEL_CALL(h);
  return h ? h->np_tf : -1;
}
int nasr_num_tensors(nasr_handle h) {
  MODEL_CALL(h);
  return h ? (int)h->tensors.size() : -1;
}

int nasr_tensor_info(nasr_handle h, int idx, char name[64], int64_t* offset, int64_t* rows, int64_t* cols) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (idx < 0 || idx >= (int)h->tensors.size()) return h->fail(NASR_ERR_ARG, "tensor index out of range");
  const TensorInfo& t = h->tensors[idx];
  if (name) {
    strncpy(name, t.name.c_str(), 63);
    name[63] = 0;
  }
  if (offset) *offset = t.offset;
  if (rows) *rows = t.rows;
  if (cols) *cols = t.cols;
  return NASR_OK;
}

int nasr_set_params(nasr_handle h, const float* flat, int64_t n) {
  MODEL_CALL(h);
  if (!h || !flat) return NASR_ERR_ARG;
  if (n != h->np_tf) return h->fail(NASR_ERR_ARG, "nasr_set_params: expected " + std::to_string(h->np_tf) + " floats");
  HIPCHK(h, hipSetDevice(h->device));
  int rc = scatter_to_device(h, flat, h->P);
  if (rc) return rc;
  rc = repack(h);
  if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(h->st));
  return NASR_OK;
}

int nasr_get_params(nasr_handle h, float* flat, int64_t n) {
  MODEL_CALL(h);
  if (!h || !flat) return NASR_ERR_ARG;
  if (n != h->np_tf) return h->fail(NASR_ERR_ARG, "nasr_get_params: wrong length");
  HIPCHK(h, hipSetDevice(h->device));
  return gather_from_device(h, h->P, flat);
}

int nasr_set_adam_state(nasr_handle h, const float* m, const float* v, int64_t n, int64_t step) {
  MODEL_CALL(h);
  if (!h || !m || !v) return NASR_ERR_ARG;
  if (n != h->np_tf || step < 0) return h->fail(NASR_ERR_ARG, "nasr_set_adam_state: wrong length or negative step");
  HIPCHK(h, hipSetDevice(h->device));
  int rc = scatter_to_device(h, m, h->M);
  if (rc) return rc;
  rc = scatter_to_device(h, v, h->V);
  if (rc) return rc;
  const AdamDev init{(long long)step, 0.f, 0};
  HIPCHK(h, hipMemcpyAsync(h->adam_dev, &init, sizeof(init), hipMemcpyHostToDevice, h->st));
  HIPCHK(h, hipStreamSynchronize(h->st));
  return NASR_OK;
}

int nasr_get_adam_state(nasr_handle h, float* m, float* v, int64_t n, int64_t* step) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (n != h->np_tf) return h->fail(NASR_ERR_ARG, "nasr_get_adam_state: wrong length");
  HIPCHK(h, hipSetDevice(h->device));
  int rc = NASR_OK;
  if (m) rc = gather_from_device(h, h->M, m);
  if (!rc && v) rc = gather_from_device(h, h->V, v);
  if (step) {
    AdamDev d{};
    HIPCHK(h, hipMemcpyAsync(&d, h->adam_dev, sizeof(d), hipMemcpyDeviceToHost, h->st));
    if (int rc2 = sync_checked(h)) return rc2;
    *step = d.step;
  }
  return rc;
}

int nasr_set_learning_rate(nasr_handle h, float lr) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  h->lr = lr;
  return NASR_OK;
}

int nasr_get_learning_rate(nasr_handle h, float* lr) {
  MODEL_CALL(h);
  if (!h || !lr) return NASR_ERR_ARG;
  *lr = h->lr;
  return NASR_OK;
}

// ---- parameter averaging (optim.hip) ---------------------------------------------------------------
int nasr_set_ema(nasr_handle h, float decay) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (!(decay >= 0.f && decay < 1.f)) return h->fail(NASR_ERR_ARG, "nasr_set_ema: decay must be 0 (off) or a number in (0,1)");
  HIPCHK(h, hipSetDevice(h->device));
  if (decay == 0.f) {
    NOT_EMA_LIVE(h);
    if (h->E) {
      HIPCHK(h, hipStreamSynchronize(h->st));   // a step in flight still writes E
      h->E.reset();
      h->ema_dev.reset();
    }
    h->ema_decay = 0.f;
    return NASR_OK;
  }
  if (!h->E) {   // the first switch-on: the average starts at the parameters (TF's initial shadow value), no update yet
    const size_t nb = (size_t)h->np_int * 4;
    if (hipMalloc(h->E.out(), nb) != hipSuccess || hipMalloc(h->ema_dev.out(), sizeof(EmaDev)) != hipSuccess) {
      h->E.reset();
      h->ema_dev.reset();
      (void)hipGetLastError();
      return h->fail(NASR_ERR_HIP, "nasr_set_ema: hipMalloc of the averaged parameters failed");
    }
    HIPCHK(h, hipMemcpyAsync(h->E, h->P, nb, hipMemcpyDeviceToDevice, h->st));
    HIPCHK(h, hipMemsetAsync(h->ema_dev, 0, sizeof(EmaDev), h->st));
  }
  h->ema_decay = decay;
  return NASR_OK;
}

int nasr_get_ema(nasr_handle h, float* decay, int64_t* updates, int* live) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (decay) *decay = h->ema_decay;
  if (live) *live = h->ema_live ? 1 : 0;
  if (updates) {
    *updates = 0;
    if (h->E) {
      HIPCHK(h, hipSetDevice(h->device));
      EmaDev d{};
      HIPCHK(h, hipMemcpyAsync(&d, h->ema_dev, sizeof(d), hipMemcpyDeviceToHost, h->st));
      if (int rc = sync_checked(h)) return rc;
      *updates = d.updates;
    }
  }
  return NASR_OK;
}

int nasr_get_ema_state(nasr_handle h, float* flat, int64_t n, int64_t* updates) {
  MODEL_CALL(h);
  if (!h || !flat) return NASR_ERR_ARG;
  if (!h->E) return h->fail(NASR_ERR_STATE, "nasr_get_ema_state: averaging is off (nasr_set_ema)");
  if (n != h->np_tf) return h->fail(NASR_ERR_ARG, "nasr_get_ema_state: wrong length");
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = gather_from_device(h, h->E, flat)) return rc;
  return updates ? nasr_get_ema(h, nullptr, updates, nullptr) : NASR_OK;
}

int nasr_set_ema_state(nasr_handle h, const float* flat, int64_t n, int64_t updates) {
  MODEL_CALL(h);
  if (!h || !flat) return NASR_ERR_ARG;
  if (!h->E) return h->fail(NASR_ERR_STATE, "nasr_set_ema_state: averaging is off (nasr_set_ema)");
  NOT_EMA_LIVE(h);
  if (n != h->np_tf || updates < 0) return h->fail(NASR_ERR_ARG, "nasr_set_ema_state: wrong length or negative updates");
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = scatter_to_device(h, flat, h->E)) return rc;
  const EmaDev init{(long long)updates, 0.f};
  HIPCHK(h, hipMemcpyAsync(h->ema_dev, &init, sizeof(init), hipMemcpyHostToDevice, h->st));
  HIPCHK(h, hipStreamSynchronize(h->st));
  return NASR_OK;
}

int nasr_ema_swap(nasr_handle h) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (!h->E) return h->fail(NASR_ERR_STATE, "nasr_ema_swap: averaging is off (nasr_set_ema)");
  HIPCHK(h, hipSetDevice(h->device));
  launch_swap16(h->P, h->E, h->np_int, h->st);
  HIPCHK(h, hipGetLastError());
  if (int rc = repack(h)) return rc;   // the operand images follow the parameters, as behind every Adam step
  h->have_fwd = false;                 // (logits of the other parameters)
  h->ema_live = !h->ema_live;
  return NASR_OK;
}

int nasr_logit_frames(nasr_handle h, int T) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  switch (h->family) {
    case Family::Las: return h->fail(NASR_ERR_STATE, "nasr_logit_frames: a LAS handle has no CTC logit frames");
    case Family::Lstm: return lstm_logit_frames(h, skip_frames(T, lstm_frame_skip(h)));   // T: input frames
    default: return T;
  }
}

int nasr_upload_batch(nasr_handle h, const float* feats, const int32_t* seq_len, const int32_t* labels,
                      const int32_t* label_len, int B, int T, int Lmax) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  return upload(h, stacked_batch(feats, seq_len, labels, label_len, B, T, Lmax));
}

int nasr_upload_batch_context(nasr_handle h, const float* centre, const float* pad_value, int numcontext, int numcep,
                              const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T,
                              int Lmax) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (!centre) return h->fail(NASR_ERR_ARG, "null input buffer");
  return upload(h, centre_batch(centre, pad_value, numcontext, numcep, seq_len, labels, label_len, B, T, Lmax, nullptr));
}

int nasr_upload_batch_context_aug(nasr_handle h, const float* centre, const float* pad_value, int numcontext, int numcep,
                                  const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T,
                                  int Lmax, const nasr_batch_aug* aug) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (!centre) return h->fail(NASR_ERR_ARG, "null input buffer");
  return upload(h, centre_batch(centre, pad_value, numcontext, numcep, seq_len, labels, label_len, B, T, Lmax, aug));
}

int nasr_stage_batch(nasr_handle h, const float* feats, const int32_t* seq_len, const int32_t* labels,
                     const int32_t* label_len, int B, int T, int Lmax, int* ticket) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  return stage(h, stacked_batch(feats, seq_len, labels, label_len, B, T, Lmax), ticket);
}

int nasr_stage_batch_context(nasr_handle h, const float* centre, const float* pad_value, int numcontext, int numcep,
                             const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T,
                             int Lmax, int* ticket) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (!centre) return h->fail(NASR_ERR_ARG, "null input buffer");
  return stage(h, centre_batch(centre, pad_value, numcontext, numcep, seq_len, labels, label_len, B, T, Lmax, nullptr), ticket);
}

int nasr_commit_batch(nasr_handle h, int ticket) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  BatchSlot* s = slot_of_ticket(h, ticket);
  if (!s) return h->fail(NASR_ERR_STATE, "nasr_commit_batch: no staged batch behind this ticket");
  const int rc = slot_commit(h, s);
  if (rc && h->cur != s) slot_set_state(h, s, SLOT_FREE);
  return rc;
}

int nasr_discard_batch(nasr_handle h, int ticket) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  BatchSlot* s = slot_of_ticket(h, ticket);
  if (!s) return h->fail(NASR_ERR_STATE, "nasr_discard_batch: no staged batch behind this ticket");
  slot_set_state(h, s, SLOT_FREE);
  return NASR_OK;
}

int nasr_compute_grads(nasr_handle h) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  NOT_EMA_LIVE(h);
  if (!h->resident) return h->fail(NASR_ERR_STATE, "no resident batch");
  if (h->kd_weight > 0.f && !h->teach_valid)   // a silently plain step would hide a broken training loop
    return h->fail(NASR_ERR_STATE, "nasr_compute_grads: distillation is on (nasr_set_distill) and the resident batch has no teacher "
                                   "logits: call nasr_set_teacher_logits or nasr_take_teacher_logits after the upload");
  HIPCHK(h, hipSetDevice(h->device));
  if (h->profiling && !h->window_open) {  // a fresh timing window per step when the batch stays resident
    h->ev_used = 0;
    h->spans.clear();
    (void)hipEventRecord(h->ev_total_a, h->st);
    h->window_open = true;
    h->total_valid = false;
  }
  rec_rearm(h);                        // (nothing to re-arm on a handle without a resident recurrence)
  const int rc = loss_pass(h, true);   // a gradient pass: training-mode batch norm, scheduled sampling
  return rc ? rc : backward(h);
}

void* nasr_grad_device_ptr(nasr_handle h) { return h && h->family != Family::Featurizer ? h->Gbase : nullptr; }
int64_t nasr_grad_device_count(nasr_handle h) {
  MODEL_CALL(h);
  return h ? h->np_int + GRAD_HEAD : -1;
}

int nasr_grad_bucket_count(nasr_handle h) {
  MODEL_CALL(h);
  return h ? (int)h->buckets.size() : NASR_ERR_ARG;
}

int nasr_grad_bucket(nasr_handle h, int i, int64_t* offset, int64_t* count) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (i < 0 || i >= (int)h->buckets.size() || !offset || !count) return h->fail(NASR_ERR_ARG, "nasr_grad_bucket: bad index");
  *offset = h->buckets[i].first;
  *count = h->buckets[i].second;
  return NASR_OK;
}

int nasr_grad_bucket_wait(nasr_handle h, int i, void* hip_stream) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (i < 0 || i >= (int)h->buckets.size()) return h->fail(NASR_ERR_ARG, "nasr_grad_bucket_wait: bad index");
  HIPCHK(h, hipStreamWaitEvent((hipStream_t)hip_stream, h->ev_bucket[i], 0));
  return NASR_OK;
}

int nasr_diag_bucket_traffic(nasr_handle h, int i, void* hip_stream, int nblocks, int passes) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (i < 0 || i >= (int)h->buckets.size() || nblocks < 1 || nblocks > 1024 || passes < 1)
    return h->fail(NASR_ERR_ARG, "nasr_diag_bucket_traffic: bad bucket index, nblocks (1..1024) or passes");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamWaitEvent((hipStream_t)hip_stream, h->ev_bucket[i], 0));
  launch_ring_standin(h->Gbase + h->buckets[i].first, h->buckets[i].second, nblocks, passes, (hipStream_t)hip_stream);
  HIPCHK(h, hipGetLastError());
  return NASR_OK;
}

int nasr_apply_adam(nasr_handle h, float grad_scale) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  NOT_EMA_LIVE(h);
  if (!h->have_grads) return h->fail(NASR_ERR_STATE, "nasr_apply_adam without gradients");
  HIPCHK(h, hipSetDevice(h->device));
  {
    PhaseScope ps(h, PH_ADAM);
    if (h->max_grad_norm > 0.f)   // the norm of the (all-reduced) gradient first; its second stage decides the step on the device
      launch_adam_clipped(h->P, h->M, h->V, h->G, h->np_int, h->adam_dev, h->clip_dev, h->clip_part, h->lr, h->beta1,
                          h->beta2, h->epsilon, grad_scale, h->max_grad_norm, h->Gbase, h->E, h->ema_dev, h->ema_decay, h->st);
    else
      launch_adam(h->P, h->M, h->V, h->G, h->np_int, h->adam_dev, h->lr, h->beta1, h->beta2, h->epsilon, grad_scale,
                  h->Gbase, h->E, h->ema_dev, h->ema_decay, h->st);
    int rc = repack(h);
    if (rc) return rc;
    // the step's fault word as it stands now (all-reduced with the gradients): read later, without a stream sync
    h->end_cur = (h->end_cur + 1) % nasr_ctx::NEND;
    nasr_ctx::StepEnd& e = h->endw[h->end_cur];
    e.seq = ++h->stamp_seq;
    e.token = ++h->step_token;
    launch_stamp(e.stamp, e.seq, e.host, (const float*)h->Gbase, h->st);
    e.valid = true;
  }
  if (h->profiling && h->window_open) {
    (void)hipEventRecord(h->ev_total_b, h->st);
    h->window_open = false;
    h->total_valid = true;
  }
  h->have_grads = false;
  return NASR_OK;
}

int nasr_set_grad_clip(nasr_handle h, float max_norm) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (!(max_norm >= 0.f)) return h->fail(NASR_ERR_ARG, "nasr_set_grad_clip: max_norm must be 0 (off), positive or +inf");
  h->max_grad_norm = max_norm;
  return NASR_OK;
}

int nasr_get_grad_clip(nasr_handle h, float* max_norm) {
  MODEL_CALL(h);
  if (!h || !max_norm) return NASR_ERR_ARG;
  *max_norm = h->max_grad_norm;
  return NASR_OK;
}

int nasr_get_grad_clip_stats(nasr_handle h, nasr_clip_stats* out, int reset) {
  MODEL_CALL(h);
  if (!h || !out) return NASR_ERR_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  ClipDev d{};
  HIPCHK(h, hipMemcpyAsync(&d, h->clip_dev, sizeof(d), hipMemcpyDeviceToHost, h->st));
  if (reset) {   // the window: its largest norm and the three counters, the tail of ClipDev
    constexpr size_t off = offsetof(ClipDev, window_max_norm);
    HIPCHK(h, hipMemsetAsync(reinterpret_cast<char*>(h->clip_dev.get()) + off, 0, sizeof(ClipDev) - off, h->st));
  }
  if (int rc = sync_checked(h)) return rc;
  out->last_norm = d.last_norm;
  out->window_max_norm = d.window_max_norm;
  out->last_coef = d.last_coef;
  out->steps = d.steps;
  out->clipped = d.clipped;
  out->skipped = d.skipped;
  return NASR_OK;
}

int nasr_get_grads(nasr_handle h, float* flat, int64_t n) {
  MODEL_CALL(h);
  if (!h || !flat) return NASR_ERR_ARG;
  if (n != h->np_tf) return h->fail(NASR_ERR_ARG, "nasr_get_grads: wrong length");
  if (!h->have_grads) return h->fail(NASR_ERR_STATE, "nasr_get_grads without gradients");
  HIPCHK(h, hipSetDevice(h->device));
  return gather_from_device(h, h->G, flat);
}

int nasr_set_grads(nasr_handle h, const float* flat, int64_t n) {
  MODEL_CALL(h);
  if (!h || !flat) return NASR_ERR_ARG;
  if (n != h->np_tf) return h->fail(NASR_ERR_ARG, "nasr_set_grads: wrong length");
  HIPCHK(h, hipSetDevice(h->device));
  int rc = scatter_to_device(h, flat, h->G);
  if (rc) return rc;
  HIPCHK(h, hipMemsetAsync(h->Gbase, 0, GRAD_HEAD * 4, h->st));
  h->have_grads = true;
  return NASR_OK;
}

int nasr_label_error_rate(const int32_t* hyp_ids, const int32_t* hyp_lens, int hyp_stride, const int32_t* labels,
                          const int32_t* label_len, int Lmax, int B, float* ler_out) {
  if (!hyp_ids || !hyp_lens || !labels || !label_len || !ler_out || B < 1) return NASR_ERR_ARG;
  double acc = 0.0;
  std::vector<int> row;
  for (int b = 0; b < B; ++b) {
    const int n = hyp_lens[b], m = label_len[b];
    const int32_t* hy = hyp_ids + (size_t)b * hyp_stride;
    const int32_t* tr = labels + (size_t)b * Lmax;
    if (m == 0) {
      acc += n > 0 ? INFINITY : 0.0;
      continue;
    }
    row.resize((size_t)m + 1);
    for (int j = 0; j <= m; ++j) row[j] = j;
    for (int i = 1; i <= n; ++i) {
      int prev = row[0];
      row[0] = i;
      for (int j = 1; j <= m; ++j) {
        const int cur = row[j];
        const int sub = prev + (hy[i - 1] != tr[j - 1] ? 1 : 0);
        row[j] = std::min(std::min(row[j] + 1, row[j - 1] + 1), sub);
        prev = cur;
      }
    }
    acc += (double)row[m] / (double)m;
  }
  *ler_out = (float)(acc / B);
  return NASR_OK;
}

int nasr_get_loss(nasr_handle h, float* loss_out) {
  MODEL_CALL(h);
  if (!h || !loss_out) return NASR_ERR_ARG;
  // the step's fault word travels with the gradients through the all-reduce: non-zero = some rank's persistent
  // recurrence gave up, every rank's Adam launch of that step was a no-op (optim.hip) and the step is void everywhere
  float fault = 0.f;
  HIPCHK(h, hipMemcpyAsync(loss_out, h->loss.p, 4, hipMemcpyDeviceToHost, h->st));
  HIPCHK(h, hipMemcpyAsync(&fault, h->Gbase, 4, hipMemcpyDeviceToHost, h->st));
  const int rc = sync_checked(h);
  if (fault != 0.f) {
    if (rc) return rc;
    return h->fail(NASR_ERR_HIP, "this training step is void: the persistent recurrence of another rank aborted; no "
                                 "parameters were changed on any rank");
  }
  return rc;
}

int nasr_step_void(nasr_handle h, int* void_out) {
  MODEL_CALL(h);
  if (!h || !void_out) return NASR_ERR_ARG;
  float fault = 0.f;
  HIPCHK(h, hipMemcpyAsync(&fault, h->Gbase, 4, hipMemcpyDeviceToHost, h->st));
  HIPCHK(h, hipStreamSynchronize(h->st));
  (void)rec_check(h);   // a local abort: switch this handle to the per-step kernels (the message stays in last_error)
  *void_out = fault != 0.f ? 1 : 0;
  return NASR_OK;
}

int nasr_get_step_results(nasr_handle h, float* loss_out, int* fault_out, int32_t* ids_out, int32_t* lens_out) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  nasr_ctx::StepRes& r = h->res[h->res_cur];
  if (!r.valid) return h->fail(NASR_ERR_STATE, "nasr_get_step_results: no step with nasr_set_step_decode(1) has been enqueued");
  // the forward pass + CTC of the step; its backward pass may still run
  if (!wait_stamp(r.stamp, r.seq, 60.0)) return h->fail(NASR_ERR_HIP, "nasr_get_step_results: the step's results did not arrive within 60 s");
  const char* hp = static_cast<const char*>(r.host.get());
  float fault;
  memcpy(&fault, hp + 4, 4);
  if (loss_out) memcpy(loss_out, hp, 4);
  if (fault_out) *fault_out = fault != 0.f ? 1 : 0;
  if (!r.greedy) {                      // nasr_set_step_decode(h, 2): no greedy decode was run - empty hypotheses
    if (lens_out) memset(lens_out, 0, (size_t)r.B * 4);
    if (ids_out) memset(ids_out, 0, (size_t)r.B * r.Tp * 4);
    return NASR_OK;
  }
  if (lens_out) memcpy(lens_out, hp + 8, (size_t)r.B * 4);
  if (ids_out) memcpy(ids_out, hp + 8 + (size_t)r.Bp * 4, (size_t)r.B * r.Tp * 4);
  return NASR_OK;
}


int nasr_settle_step(nasr_handle h, int previous, int* void_out) {
  MODEL_CALL(h);
  if (!h || !void_out) return NASR_ERR_ARG;
  *void_out = 0;
  nasr_ctx::StepEnd& e = h->endw[previous ? (h->end_cur + nasr_ctx::NEND - 1) % nasr_ctx::NEND : h->end_cur];
  if (!e.valid) return NASR_OK;
  return settle_end(h, e, void_out);
}

int64_t nasr_step_token(nasr_handle h) {
  MODEL_CALL(h);
  return h ? h->step_token : -1;
}

int nasr_settle_token(nasr_handle h, int64_t token, int* void_out) {
  MODEL_CALL(h);
  if (!h || !void_out) return NASR_ERR_ARG;
  *void_out = 0;
  if (token <= 0 || token > h->step_token) return h->fail(NASR_ERR_ARG, "nasr_settle_token: no such step");
  for (auto& e : h->endw)
    if (e.valid && e.token == token) return settle_end(h, e, void_out);
  return h->fail(NASR_ERR_STATE, "nasr_settle_token: the library remembers the last " + std::to_string(nasr_ctx::NEND) +
                                     " optimiser steps; this token is older");
}

int nasr_resident_frames(nasr_handle h, int64_t* frames) {
  MODEL_CALL(h);
  if (!h || !frames) return NASR_ERR_ARG;
  *frames = h->resident ? h->frames : 0;
  return NASR_OK;
}

int nasr_resident_rows(nasr_handle h, int64_t* rows) {
  MODEL_CALL(h);
  if (!h || !rows) return NASR_ERR_ARG;
  *rows = !h->resident ? 0 : h->cmp_rows ? h->cmp_rows : (int64_t)h->T * h->Bp;
  return NASR_OK;
}

int nasr_train_step(nasr_handle h, const float* feats, const int32_t* seq_len, const int32_t* labels,
                    const int32_t* label_len, int B, int T, int Lmax, float* loss_out) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  NOT_EMA_LIVE(h);
  if (!labels) return h->fail(NASR_ERR_ARG, "nasr_train_step needs labels");
  int rc = upload(h, stacked_batch(feats, seq_len, labels, label_len, B, T, Lmax));
  if (rc) return rc;
  rc = nasr_compute_grads(h);
  if (rc) return rc;
  rc = nasr_apply_adam(h, 1.f);
  if (rc) return rc;
  if (loss_out) return nasr_get_loss(h, loss_out);
  return NASR_OK;
}

int nasr_forward_resident(nasr_handle h, float* logits_out) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (!h->resident) return h->fail(NASR_ERR_STATE, "no resident batch");
  const int rc = forward(h);
  if (rc) return rc;
  if (logits_out) return fetch_logits(h, logits_out);
  return nasr_synchronize(h);
}

int nasr_forward(nasr_handle h, const float* feats, const int32_t* seq_len, int B, int T, float* logits_out) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  const int rc = upload(h, stacked_batch(feats, seq_len, nullptr, nullptr, B, T, 0));
  if (rc) return rc;
  return nasr_forward_resident(h, logits_out);
}

int nasr_loss(nasr_handle h, const float* feats, const int32_t* seq_len, const int32_t* labels,
              const int32_t* label_len, int B, int T, int Lmax, float* loss_out, float* nll_out) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (!labels) return h->fail(NASR_ERR_ARG, "nasr_loss needs labels");
  const int rc = upload(h, stacked_batch(feats, seq_len, labels, label_len, B, T, Lmax));
  if (rc) return rc;
  return nasr_loss_resident(h, loss_out, nll_out);
}

int nasr_loss_resident(nasr_handle h, float* loss_out, float* nll_out) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (!h->resident || !h->cur || !h->cur->has_labels) return h->fail(NASR_ERR_STATE, "no resident batch with labels");
  const int rc = loss_pass(h, false);   // inference-mode batch norm
  if (rc) return rc;
  if (nll_out) HIPCHK(h, hipMemcpyAsync(nll_out, h->nll.p, (size_t)h->B * 4, hipMemcpyDeviceToHost, h->st));
  if (loss_out) return nasr_get_loss(h, loss_out);
  return nasr_synchronize(h);
}

int nasr_loss_and_grads(nasr_handle h, const float* feats, const int32_t* seq_len, const int32_t* labels,
                        const int32_t* label_len, int B, int T, int Lmax, float* loss_out, float* nll_out,
                        float* flat_grads_out) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (!labels) return h->fail(NASR_ERR_ARG, "nasr_loss_and_grads needs labels");
  int rc = upload(h, stacked_batch(feats, seq_len, labels, label_len, B, T, Lmax));
  if (rc) return rc;
  rc = nasr_compute_grads(h);
  if (rc) return rc;
  if (nll_out) HIPCHK(h, hipMemcpyAsync(nll_out, h->nll.p, (size_t)B * 4, hipMemcpyDeviceToHost, h->st));
  if (loss_out) {
    rc = nasr_get_loss(h, loss_out);
    if (rc) return rc;
  }
  if (flat_grads_out) return gather_from_device(h, h->G, flat_grads_out);
  return nasr_synchronize(h);
}

int nasr_greedy_decode(nasr_handle h, const float* feats, const int32_t* seq_len, int B, int T, int32_t* ids_out,
                       int32_t* lens_out) {
  MODEL_CALL(h);
  if (!h || !ids_out || !lens_out) return NASR_ERR_ARG;
  if (h->family == Family::Las) return h->fail(NASR_ERR_STATE, "nasr_greedy_decode: a LAS handle has no CTC decoder");
  const int rc = upload(h, stacked_batch(feats, seq_len, nullptr, nullptr, B, T, 0));
  if (rc) return rc;
  return nasr_greedy_decode_resident(h, ids_out, lens_out);
}

int nasr_greedy_decode_resident(nasr_handle h, int32_t* ids_out, int32_t* lens_out) {
  MODEL_CALL(h);
  if (!h || !ids_out || !lens_out) return NASR_ERR_ARG;
  if (h->family == Family::Las) return h->fail(NASR_ERR_STATE, "nasr_greedy_decode: a LAS handle has no CTC decoder");
  if (!h->resident) return h->fail(NASR_ERR_STATE, "no resident batch");
  const int rc = forward(h);
  if (rc) return rc;
  const CtcDims d = ctc_dims(h);
  launch_greedy(d, h->logits.as<float>(), h->seq_p, h->amax.as<int>(), h->ids.as<int>(), h->lens.as<int>(),
                h->st);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(lens_out, h->lens.p, (size_t)h->B * 4, hipMemcpyDeviceToHost, h->st));
  HIPCHK(h, hipMemcpyAsync(ids_out, h->ids.p, (size_t)h->B * h->Tp * 4, hipMemcpyDeviceToHost, h->st));
  return sync_checked(h);
}

// ---- forced alignment (ctc.hip (4)) ----------------------------------------------------------------
// logZ of every row, the walk and the way back over logits [Tp*Bp][Cp] on the handle's stream, in workspaces of the
// alignment's own; path and score to the host.  Lm: the stride of the label rows (>= 1), F: the longest seq_len.
static int align_run(nasr_ctx* h, const char* fn, const float* logits, const int32_t* seq_d, const int32_t* labels_d,
                     const int32_t* lablen_d, int B, int Bp, int Tp, int C, int Cp, int Lm, int F, int32_t* path_out,
                     double* score_out) {
  if (2 * Lm + 1 > 64 * 16) return h->fail(NASR_ERR_ARG, std::string(fn) + ": label length > 511 not supported by the CTC lattice kernels");
  if ((size_t)Tp * Bp * Cp * 4 >= ((size_t)1 << 32))
    return h->fail(NASR_ERR_ARG, std::string(fn) + ": T' x B x C logits beyond the lattice kernels' 32-bit offsets");
  const size_t wsw = ctc_align_ws_words(B, F, Lm);
  bool grew = false;
  if (!h->al_logz.ensure((size_t)Tp * Bp * 4, &grew) || !h->al_path.ensure((size_t)B * Tp * 4, &grew) ||
      !h->al_score.ensure((size_t)B * 8, &grew) || (wsw && !h->al_bp.ensure(wsw * 4, &grew)))
    return h->fail(NASR_ERR_HIP, std::string(fn) + ": hipMalloc of the alignment's workspaces failed");
  CtcDims d;
  d.Tp = Tp; d.B = B; d.Bp = Bp; d.C = C; d.Cp = Cp; d.Lmax = Lm; d.KS = 0; d.Tws = 0;   // (no lprobs: logZ only)
  launch_ctc_logz(d, logits, seq_d, h->al_logz.as<float>(), h->st);
  if (launch_ctc_align(d, F, logits, h->al_logz.as<float>(), labels_d, lablen_d, seq_d, h->al_bp.as<unsigned>(),
                       h->al_path.as<int>(), h->al_score.as<double>(), h->st) != 0)
    return h->fail(NASR_ERR_ARG, std::string(fn) + ": the alignment kernel refused the shape");
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(path_out, h->al_path.p, (size_t)B * Tp * 4, hipMemcpyDeviceToHost, h->st));
  HIPCHK(h, hipMemcpyAsync(score_out, h->al_score.p, (size_t)B * 8, hipMemcpyDeviceToHost, h->st));
  return sync_checked(h);
}

int nasr_ctc_align_lds(int F, int L) {
  if (F < 1 || L < 0 || L > 511) return NASR_ERR_ARG;
  return ctc_align_bp_in_lds(F, std::max(L, 1)) ? 1 : 0;
}

int nasr_ctc_align_resident(nasr_handle h, int32_t* path_out, double* score_out) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (h->family == Family::Las) return h->fail(NASR_ERR_STATE, "nasr_ctc_align_resident: a LAS handle has no CTC lattice");
  if (!path_out || !score_out) return h->fail(NASR_ERR_ARG, "nasr_ctc_align_resident: null output buffer");
  if (!h->resident || !h->cur || !h->cur->has_labels)
    return h->fail(NASR_ERR_STATE, "nasr_ctc_align_resident: no resident batch with labels");
  const int rc = forward(h);
  if (rc) return rc;
  int F = 1;
  for (int b = 0; b < h->B; ++b) F = std::max(F, (int)h->h_seq[b]);
  return align_run(h, "nasr_ctc_align_resident", h->logits.as<float>(), h->seq_p, h->labels_p, h->lablen_p, h->B, h->Bp, h->Tp,
                   h->C, h->Cp, std::max(h->Lmax, 1), F, path_out, score_out);
}

int nasr_ctc_align(nasr_handle h, const float* feats, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len,
                   int B, int T, int Lmax, int32_t* path_out, double* score_out) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (h->family == Family::Las) return h->fail(NASR_ERR_STATE, "nasr_ctc_align: a LAS handle has no CTC lattice");
  if (!labels || !path_out || !score_out) return h->fail(NASR_ERR_ARG, "nasr_ctc_align needs labels and both output buffers");
  const int rc = upload(h, stacked_batch(feats, seq_len, labels, label_len, B, T, Lmax));
  if (rc) return rc;
  return nasr_ctc_align_resident(h, path_out, score_out);
}

int nasr_ctc_align_logits(nasr_handle h, const float* logits, const int32_t* seq_len, const int32_t* labels,
                          const int32_t* label_len, int B, int Tp, int C, int Lmax, int32_t* path_out, double* score_out) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (h->family == Family::Las) return h->fail(NASR_ERR_STATE, "nasr_ctc_align_logits: a LAS handle has no CTC lattice");
  if (!logits || !seq_len || !label_len || (Lmax > 0 && !labels) || !path_out || !score_out)
    return h->fail(NASR_ERR_ARG, "nasr_ctc_align_logits: null buffer");
  if (C < 2) return h->fail(NASR_ERR_ARG, "nasr_ctc_align_logits: need num_classes >= 2 (a label and the blank)");
  if (Lmax < 0) return h->fail(NASR_ERR_ARG, "nasr_ctc_align_logits: Lmax < 0");
  if (Lmax > 511) return h->fail(NASR_ERR_ARG, "nasr_ctc_align_logits: label length > 511 not supported by the CTC lattice kernels");
  static const int32_t no_label = 0;
  int rc = validate_batch(h, seq_len, Lmax > 0 ? labels : &no_label, label_len, B, Tp, Lmax, C);   // before anything is launched
  if (rc) return rc;
  const int Bp = rup(B, 16), Cp = rup(C, 32), Lm = std::max(Lmax, 1);
  if ((size_t)Tp * Bp * Cp * 4 >= ((size_t)1 << 32))
    return h->fail(NASR_ERR_ARG, "nasr_ctc_align_logits: T' x B x C logits beyond the lattice kernels' 32-bit offsets");
  HIPCHK(h, hipSetDevice(h->device));
  // the caller's logits in the kernels' layout (rows t*Bp + b of Cp floats), and seq [Bp] | lablen [Bp] | labels [B][Lm]
  std::vector<float> lg((size_t)Tp * Bp * Cp, 0.f);
  for (int t = 0; t < Tp; ++t)
    for (int b = 0; b < B; ++b)
      memcpy(lg.data() + ((size_t)t * Bp + b) * Cp, logits + ((size_t)t * B + b) * C, (size_t)C * 4);
  std::vector<int32_t> meta((size_t)2 * Bp + (size_t)B * Lm, 0);
  int F = 1;
  for (int b = 0; b < B; ++b) {
    meta[b] = seq_len[b];
    meta[Bp + b] = label_len[b];
    F = std::max(F, (int)seq_len[b]);
    if (Lmax > 0) memcpy(meta.data() + 2 * Bp + (size_t)b * Lm, labels + (size_t)b * Lmax, (size_t)Lmax * 4);
  }
  bool grew = false;
  if (!h->al_logits.ensure(lg.size() * 4, &grew) || !h->al_meta.ensure(meta.size() * 4, &grew))
    return h->fail(NASR_ERR_HIP, "nasr_ctc_align_logits: hipMalloc of the alignment's workspaces failed");
  // from the first copy on every way out passes a stream synchronise: the copies read lg and meta
  auto run = [&]() -> int {
    HIPCHK(h, hipMemcpyAsync(h->al_logits.p, lg.data(), lg.size() * 4, hipMemcpyHostToDevice, h->st));
    HIPCHK(h, hipMemcpyAsync(h->al_meta.p, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, h->st));
    const int32_t* md = h->al_meta.as<int32_t>();
    return align_run(h, "nasr_ctc_align_logits", h->al_logits.as<float>(), md, md + 2 * Bp, md + Bp, B, Bp, Tp, C, Cp, Lm, F,
                     path_out, score_out);
  };
  rc = run();
  if (rc) (void)hipStreamSynchronize(h->st);
  return rc;
}

int nasr_resident_shape(nasr_handle h, int* B, int* T) {
  MODEL_CALL(h);
  if (!h || !B || !T) return NASR_ERR_ARG;
  *B = h->resident ? h->B : 0;
  *T = h->resident ? h->Tin : 0;   // the caller's input frames, whatever the frame skip
  return NASR_OK;
}

int nasr_set_step_decode(nasr_handle h, int enabled) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  if (h->family == Family::Las && (enabled & 1)) return h->fail(NASR_ERR_STATE, "nasr_set_step_decode: a LAS handle has no greedy CTC pass");
  h->step_decode = enabled != 0;
  h->step_greedy = (enabled & 1) != 0;
  h->step_logits = (enabled & 2) != 0;
  return NASR_OK;
}

int nasr_get_step_logits(nasr_handle h, float* logits_out) {
  MODEL_CALL(h);
  if (!h || !logits_out) return NASR_ERR_ARG;
  nasr_ctx::StepRes& r = h->res[h->res_cur];
  if (!r.valid || !r.logits)
    return h->fail(NASR_ERR_STATE, "nasr_get_step_logits: no step with nasr_set_step_decode(h, 3) has been enqueued");
  if (!wait_stamp(r.stamp, r.seq, 60.0)) return h->fail(NASR_ERR_HIP, "nasr_get_step_logits: the step's results did not arrive within 60 s");
  HIPCHK(h, hipEventSynchronize(r.ev_lg));          // the logits travel on a stream of their own (ctc_forward)
  const size_t ids_bytes = 8 + (size_t)r.Bp * 4 + (size_t)r.B * r.Tp * 4;
  const float* src = reinterpret_cast<const float*>(static_cast<const char*>(r.host.get()) + (ids_bytes + 255) / 256 * 256);
  for (int t = 0; t < r.Tp; ++t)
    for (int b = 0; b < r.B; ++b)
      memcpy(logits_out + ((size_t)t * r.B + b) * h->C, src + ((size_t)t * r.Bp + b) * h->Cp, (size_t)h->C * 4);
  return NASR_OK;
}

int nasr_get_decoded(nasr_handle h, int32_t* ids_out, int32_t* lens_out) {
  MODEL_CALL(h);
  if (!h || !ids_out || !lens_out) return NASR_ERR_ARG;
  if (!h->have_decoded) return h->fail(NASR_ERR_STATE, "nasr_get_decoded: no decoded step (enable nasr_set_step_decode)");
  HIPCHK(h, hipMemcpyAsync(lens_out, h->lens.p, (size_t)h->B * 4, hipMemcpyDeviceToHost, h->st));
  HIPCHK(h, hipMemcpyAsync(ids_out, h->ids.p, (size_t)h->B * h->Tp * 4, hipMemcpyDeviceToHost, h->st));
  return sync_checked(h);
}

int nasr_set_profiling(nasr_handle h, int enabled) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  h->profiling = enabled != 0;
  h->ev_used = 0;
  h->spans.clear();
  h->window_open = false;
  h->total_valid = false;
  return NASR_OK;
}

int nasr_get_phase_times(nasr_handle h, nasr_phase_times* out) {
  MODEL_CALL(h);
  if (!h || !out) return NASR_ERR_ARG;
  HIPCHK(h, hipStreamSynchronize(h->st));
  float acc[PH_COUNT] = {0};
  for (const auto& s : h->spans) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) acc[s.ph] += ms;
  }
  nasr_phase_times t;
  memset(&t, 0, sizeof(t));
  t.pack_ms = acc[PH_PACK]; t.xproj_ms = acc[PH_XPROJ]; t.rec_fwd_ms = acc[PH_RECF]; t.proj_ctc_ms = acc[PH_PROJCTC];
  t.proj_bwd_ms = acc[PH_PROJB]; t.rec_bwd_ms = acc[PH_RECB]; t.wgrad_ms = acc[PH_WGRAD]; t.adam_ms = acc[PH_ADAM];
  float tot = 0.f;
  if (h->total_valid && hipEventElapsedTime(&tot, h->ev_total_a, h->ev_total_b) == hipSuccess) t.total_ms = tot;
  (void)hipGetLastError();
  t.rec_fwd_launches = h->n_fwd_launch;
  t.rec_bwd_launches = h->n_bwd_launch;
  *out = t;
  return NASR_OK;
}

int nasr_set_graph_mode(nasr_handle h, int enabled) {
  MODEL_CALL(h);
  if (!h) return NASR_ERR_ARG;
  h->graph_mode = enabled != 0;
  if (!h->graph_mode) drop_graphs(h);
  return NASR_OK;
}

}  // extern "C"
