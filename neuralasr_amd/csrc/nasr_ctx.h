// nasr_ctx.h — what the translation units behind include/nasr.h share: the handle (struct nasr_ctx: what every handle kind
// has - parameters and optimiser state, batch slots and the resident batch, the CTC head's buffers, streams / events - and
// one pointer to each family's own state), small helpers, and the functions they call in each other (internal, C++).
//   nasr_lstm.h      struct LstmState: what a (Bi)LSTM CTC handle holds beyond nasr_ctx, and the functions that work on it;
//                    included only by the files marked (L), so that nothing else can touch that state
//   nasr_lstm.hip    (L) the LSTM-family handle: its set-up (lstm_create), LstmStateDelete, the ABI calls only it answers
//   nasr_layout.hip  (L) parameter layout, TF <-> internal maps, operand images (repack); host <-> device parameter copies,
//                    the stamp and publish kernels
//   nasr_rec.hip     (L) the recurrence's kind: create-time set-up and census, resident launches, abort check, re-arming
//   nasr_batch.hip   (L) batch buffers and slots: upload, stage / commit; ensure_shape's switch and its LSTM side
//   nasr_pass.hip    (L) forward, CTC, backward: the orchestration of one step on the handle's streams; the switches of
//                    forward, loss_pass and backward and their LSTM sides
//   nasr_stream.hip  (L) streaming sessions (nasr_stream_*): recurrent state that survives between chunks
//   nasr_api.hip     the C ABI entry points that serve every family (and nasr_create's reading of the environment); what the
//                    create calls share (handle_open, alloc_param_buffers, handle_finish)
//   nasr_distill.hip distillation beside the CTC loss (nasr_set_distill, teacher logits from another handle); both CTC families
//   nasr_comm.hip    RCCL bound with dlopen: nasr_comm_*
//   nasr_wavenet.hip the WaveNet handle (nasr_create_wavenet): its layout, buffers, BN state and pass
//   nasr_las.hip     the LAS handle (nasr_create_las): its layout, buffers, sampling state and pass
//   nasr_fz.hip      the featurizer handle (nasr_create_featurizer): the front end's tables, buffers, plans and calls, over
//                    the kernels of mfcc.hip, resample.hip and wave_aug.hip; what a stream session needs of it: nasr_fz.h
#pragma once
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <sched.h>
#include <unistd.h>

#include <chrono>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/nasr.h"
#include "kernels.h"

namespace nasr_impl {
using namespace nasr;

extern std::string g_create_error;
// nasr_last_error: the message of the calling thread's last failed call (nasr_stage_batch* may fail on a loader thread
// while the training thread is inside another call of the same handle: neither sees nor overwrites the other's text)
extern thread_local std::string t_err;
extern thread_local const void* t_err_handle;

inline int rup(int x, int m) { return (x + m - 1) / m * m; }

// Owners of the handle's HIP resources: each releases what it holds when it goes (nasr_destroy ends in `delete h`) and
// converts to the raw pointer / handle, so use sites read h->P, h->Gbase + GRAD_HEAD, h->ev_snap as they would a raw
// member.  out() releases what is held and hands the slot to a create call: hipMalloc(h->P.out(), bytes).
template <typename T, hipError_t (*Free)(T)>
class Owned {
 public:
  Owned() = default;
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  Owned(Owned&& o) noexcept : v_(o.v_) { o.v_ = T{}; }
  Owned& operator=(Owned&& o) noexcept { std::swap(v_, o.v_); return *this; }
  ~Owned() { reset(); }
  void reset() {
    if (v_) (void)Free(v_);
    v_ = T{};
  }
  T* out() { reset(); return &v_; }
  T get() const { return v_; }
  operator T() const { return v_; }

 private:
  T v_{};
};
template <typename T> hipError_t free_device(T* p) { return hipFree(p); }
template <typename T> hipError_t free_pinned(T* p) { return hipHostFree(p); }
template <typename T> using DevPtr = Owned<T*, free_device<T>>;     // hipMalloc
template <typename T> using Pinned = Owned<T*, free_pinned<T>>;     // hipHostMalloc
using Event = Owned<hipEvent_t, hipEventDestroy>;

// A stream the handle made (out()) and destroys, or the caller's (borrow()), which outlives the handle.
class Stream {
 public:
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() { reset(); }
  void reset() {
    if (s_ && own_) (void)hipStreamDestroy(s_);
    s_ = nullptr;
    own_ = false;
  }
  hipStream_t* out() { reset(); own_ = true; return &s_; }
  void borrow(hipStream_t s) { reset(); s_ = s; }
  operator hipStream_t() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
  bool own_ = false;
};

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
  ~DevBuf() { release(); }
  bool ensure(size_t bytes, bool* grew) {
    if (bytes <= cap) return true;
    release();
    size_t want = bytes + bytes / 8;  // head room: fewer re-allocations for ragged T
    if (hipMalloc(&p, want) != hipSuccess) {
      if (hipMalloc(&p, bytes) != hipSuccess) return false;
      want = bytes;
    }
    cap = want;
    if (grew) *grew = true;
    return true;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <typename T>
  T* as() const { return reinterpret_cast<T*>(p); }
};

struct TensorInfo {
  std::string name;
  int64_t offset, rows, cols;
};

enum Phase { PH_PACK = 0, PH_XPROJ, PH_RECF, PH_PROJCTC, PH_PROJB, PH_RECB, PH_WGRAD, PH_ADAM, PH_COUNT };

constexpr int GRAD_HEAD = 32;   // floats in front of the gradients (h->G = h->Gbase + GRAD_HEAD); [0] = fault word of the step
constexpr int MAX_BUCKETS = 16;

// One uploaded batch: the caller's arrays in HBM (features as given, or their centre slice + pad values) and the small
// integer arrays of the step packed into one "meta" buffer, with pinned host mirrors.  One slot is the
// resident batch, others take the NEXT batches while the step runs (nasr_stage_batch: copies on the handle's copy
// stream from pinned memory), so the upload of dataset.py:33-40's next batch leaves the timed step.
constexpr int NSLOT = 4;           // the resident batch + up to NSTAGE staged ahead + one always free for a synchronous upload
constexpr int NSTAGE = 2;
enum SlotState { SLOT_FREE = 0, SLOT_FILLING, SLOT_STAGED, SLOT_RESIDENT };
struct BatchSlot {
  DevBuf dfeats, dmeta;
  Pinned<void> hfeats, hmeta;
  size_t hfeats_cap = 0, hmeta_cap = 0;
  Event ev_copy, ev_released;
  bool copy_valid = false, released_valid = false;
  int state = SLOT_FREE;
  unsigned gen = 0;                              // ticket = slot index | gen << 8
  // shape and layout of what is in it
  int B = 0, T = 0, Lmax = 0, Bp = 0, Tp = 0, ctx = 0, ncep = 0;
  bool has_labels = false, centre = false;
  int64_t frames = 0;
  // Frame skip (nasr_set_frame_skip as it stood when the slot was filled; 1 for a stream chunk, whose rows
  // the session has skipped already).  T, frames and dfeats are the caller's INPUT frames; Tn = skip_frames(T, skip) and
  // nframes count the frames the network sees, and everything the meta block lays out is in those: o_seq holds the network
  // lengths, o_seqin the input lengths beside them, which only the three feature movers read.
  int skip = 1, Tn = 0;
  int64_t nframes = 0;
  size_t o_seqin = 0;
  size_t o_seq = 0, o_lablen = 0, o_labels = 0, o_cstart = 0, o_cpos = 0, o_rowmap = 0;   // int offsets into meta
  size_t o_vrow = 0, o_vprev = 0, o_vnext = 0;   // compacted rows of a ragged batch (Rv of them, padded to Rvp with -1), or unused
  int Rv = 0, Rvp = 0;
  bool cmp = false;
  // latency-controlled training (nasr_set_chunking as it stood when the slot was filled; lcC = 0: a whole-utterance batch):
  // the compacted rows above are then the rows of the utterances' windows, and o_wlen holds wlen [lcK][Bp]
  int lcC = 0, lcR = 0, lcK = 0, lcW = 0;        // lcW = min(lcC + lcR, T) rows per window, lcK windows
  bool chunk = false;                            // a chunk of a stream session (BatchSrc::chunk)
  size_t o_wlen = 0;
  size_t nmeta = 0, nfeat = 0;                   // int32s of meta, floats of dfeats
  // SpecAugment masks of a centre-form batch (nasr_batch_aug): [B][aug_nm] of {t0, tw, f0, fw} at o_aug, or none
  size_t o_aug = 0;
  int aug_nm = 0, aug_sw = 0;
  bool masked = false;
  int32_t* meta_d() const { return dmeta.as<int32_t>(); }
};

// which create call made the handle: what the common calls run on it, and which of the state pointers below it owns
enum class Family { Lstm, WaveNet, Las, Featurizer };

// What a WaveNet handle holds beyond the common parts (nasr_wavenet.hip); NULL on every other handle.
struct WnState;
struct WnStateDelete { void operator()(WnState* w) const; };
// What a featurizer handle holds (nasr_fz.hip); NULL on every model handle.
struct FzState;
struct FzStateDelete { void operator()(FzState* f) const; };
// What a LAS handle holds beyond the common parts (nasr_las.hip); NULL on every other handle.
struct LasState;
struct LasStateDelete { void operator()(LasState* s) const; };
// What a handle of the (Bi)LSTM CTC family holds beyond the common parts (nasr_lstm.h, nasr_lstm.hip); NULL on every other handle.
struct LstmState;
struct LstmStateDelete { void operator()(LstmState* s) const; };

// The front end of a stream session that takes samples (nasr_fz.hip: nasr_stream_attach_audio); NULL while the session is
// fed finished frames.
struct FzStream;
struct FzStreamDelete { void operator()(FzStream* f) const; };

}  // namespace nasr_impl

// (internal header: the translation units behind the ABI use both namespaces unqualified)
using namespace nasr;
using namespace nasr_impl;

struct nasr_ctx {

  Family family = Family::Lstm;
  std::unique_ptr<WnState, WnStateDelete> wn;   // a WaveNet handle (nasr_create_wavenet)
  std::unique_ptr<FzState, FzStateDelete> fz;   // a featurizer handle (nasr_create_featurizer): no model at all
  std::unique_ptr<LasState, LasStateDelete> las;   // a LAS handle (nasr_create_las)
  int device = 0;
  Stream st;
  // in-library gradient exchange (nasr_comm_*): one RCCL rank per handle, collectives on a side stream
  void* comm = nullptr;                  // ncclComm_t
  // nasr_comm_mean's own communicator (ncclCommSplit of `comm`, same ranks) and stream: the two host floats of a step do
  // not queue up behind the step's gradient buckets.  NULL (old librccl): the mean shares `comm` and waits for them.
  void* comm2 = nullptr;
  Stream comm_st2;
  int comm_rank = 0, comm_n = 1;
  Stream comm_st;
  Event ev_comm;
  DevPtr<float> comm_scratch;            // 64 floats for nasr_comm_mean

  // what every model has: the feature and class widths, the flat parameters in the TF order and in the padded internal one
  int F, Fp, C, Cp;
  int64_t np_int = 0;
  std::vector<TensorInfo> tensors;
  int64_t np_tf = 0;
  std::vector<int32_t> tf2int;          // TF flat index -> internal flat index

  DevPtr<float> P, M, V;
  float* G = nullptr;                        // Gbase + GRAD_HEAD
  DevPtr<float> Gbase;                       // allocation behind G: [GRAD_HEAD floats, [0] = fault word][np_int gradients]
  // gradient buckets: (offset, count) in floats from Gbase, in the order backward() completes them; one event each
  std::vector<std::pair<int64_t, int64_t>> buckets;
  std::vector<Event> ev_bucket;
  // Adam's step count t lives ON THE DEVICE (AdamDev, optim.hip): the launch that finds the step's fault word set leaves
  // it alone, so a void step never enters the bias correction - whenever the host learns about it.
  DevPtr<AdamDev> adam_dev;
  float lr;
  float beta1 = 0.f, beta2 = 0.f, epsilon = 0.f;   // the optimiser's other hyper-parameters, from the create call's cfg
  // Global-norm gradient clipping (nasr_set_grad_clip; 0 = off, the default: nasr_apply_adam then launches what it always
  // did).  The norm, the decision and the counters live on the device beside AdamDev, so the step stays asynchronous.
  float max_grad_norm = 0.f;
  DevPtr<ClipDev> clip_dev;
  DevPtr<double> clip_part;                  // GRAD_SUMSQ_MAX_BLOCKS partial sums of squares
  // Parameter averaging (nasr_set_ema; ema_decay = 0 = off, the default: E and ema_dev are not allocated and
  // nasr_apply_adam launches what it always did).  E: a second parameter image [np_int], updated inside the Adam sweep;
  // its update count lives on the device beside AdamDev.  ema_live: nasr_ema_swap has exchanged the CONTENTS of P and E -
  // P holds the average (every offset into h->P stays good), E the training parameters, and nothing may train.
  float ema_decay = 0.f;
  bool ema_live = false;
  DevPtr<float> E;
  DevPtr<EmaDev> ema_dev;
  // Results of a step without waiting for its end (nasr_get_step_results): loss, the fault word as it stands after the
  // forward pass, and the greedy decode are copied to pinned memory right behind the CTC forward kernels; the fault
  // word at the END of a step is copied behind its Adam launch (nasr_settle_step).  Two slots each: the host may be
  // one step ahead of the device.
  struct StepRes { Pinned<void> host; size_t cap = 0; Pinned<uint32_t> stamp; uint32_t seq = 0; bool valid = false; int B = 0, Bp = 0, Tp = 0; bool logits = false, greedy = false;
                   Event ev_lg; };   // ev_lg: the step's logits have landed in host memory (stream d2h)
  StepRes res[2];
  int res_cur = 0;
  struct StepEnd { Pinned<float> host; uint32_t* stamp = nullptr; uint32_t seq = 0; bool valid = false; int64_t token = 0; };   // stamp: inside host
  static constexpr int NEND = 4;             // steps whose end the host may still ask about (nasr_settle_token)
  StepEnd endw[NEND];
  int end_cur = 0;
  int64_t step_token = 0;                    // sequence number of the optimiser step enqueued last
  uint32_t stamp_seq = 0;

  // resident batch
  bool resident = false, have_grads = false, have_fwd = false;
  int B = 0, Bp = 0, T = 0, Lmax = 0, Tp = 0, KS = 1;   // T: the frames the network sees (the slot's Tn)
  int Tin = 0;                               // the caller's input frames (nasr_resident_shape); T again without a frame skip
  int64_t frames = 0;                        // input frames (nasr_resident_frames)
  std::vector<int32_t> h_seq;
  BatchSlot slots[NSLOT];
  BatchSlot* cur = nullptr;                  // the resident batch
  Stream cst;                                // copy stream of nasr_stage_batch
  Stream d2h;                                // the step's logits leave on this one, from a snapshot (ctc_forward)
  Event ev_snap;
  DevBuf logits_snap;
  std::mutex slot_mu;                        // slot states (nasr_stage_batch may run on a loader thread)
  int slot_rr = 0;
  // device arrays of the resident batch (inside cur->dmeta / cur->dfeats)
  int32_t *seq_p = nullptr, *lablen_p = nullptr, *labels_p = nullptr, *cstart_p = nullptr, *cpos_p = nullptr,
          *rowmap_p = nullptr;
  // Ragged batches (dataset.py:75-77 pads every utterance to the batch maximum): when at least 15 % of the T x Bp frame rows
  // are padding, the plane passes and GEMMs of a plain (Bi)LSTM stack work on the COMPACTED rows - only the frames t < seq_len[b],
  // time-major - and scatter their results back (split passes gather by vrow, GEMM epilogues scatter by it; vprev / vnext =
  // the row of the frame before / after each compacted row, -1 at an utterance's first / last frame: the h_{t-1} operand of
  // the recurrent weight gradient).  cmp_rows = Rv (0: no compaction for the resident batch, as on every handle of another
  // family).  slot_commit sets these from the slot on every handle and nasr_resident_rows reads cmp_rows: they describe the
  // resident batch, as the BatchSlot's fields do; whether a handle compacts at all is LstmState's.
  int cmp_rows = 0, cmp_rows_p = 0;
  int32_t *vrow_p = nullptr, *vprev_p = nullptr, *vnext_p = nullptr;
  int32_t* wlen_p = nullptr;                 // [K][Bp] rows of every window of a chunked batch (nasr_set_chunking)

  DevBuf ctcprobs, ctckexp;                  // emission rows and column offsets of the CTC lattice (ctc.hip (2b))
  // the features, time-major and padded; the CTC head's buffers; the slab workspace of gemm_f32
  DevBuf seqbuf, X0, logits, logz, alpha, beta, aoff, boff, logp, nll, loss, slabs, amax, ids, lens;
  // forced alignment (nasr_ctc_align*): workspaces of its own, sized at the first call that needs them - its logZ rows, the
  // back-pointers that do not fit in LDS, path and score; and for nasr_ctc_align_logits the caller's logits and labels
  DevBuf al_logz, al_bp, al_path, al_score, al_logits, al_meta;

  // distillation (nasr_set_distill; kd_weight = 0 = off: nothing below is allocated or launched).
  // teach: the teacher's logits of the resident batch [Tp*Bp][Cp], never written by a step; kd_grad: the term's logit
  // gradient from the loss pass until the backward pass adds it; kd_rows / kd_sum: the rows' KL and its sums per
  // utterance (double [B]); kd_parts: {CTC, KD} of the last loss pass with the term, then the teacher's fault word.
  float kd_weight = 0.f, kd_tau = 1.f;
  bool teach_valid = false;                  // teach holds logits for the resident batch (slot_commit drops them)
  bool kd_live = false;                      // the last loss pass added the term
  DevBuf teach, kd_grad, kd_rows, kd_sum, kd_parts;
  Event ev_teach_ready, ev_teach_taken;      // nasr_take_teacher_logits: the order between the two handles' streams

  bool graph_mode = true;                    // nasr_set_graph_mode: read by every family's pass (the graph cache: LstmState)
  bool step_decode = false, step_logits = false, have_decoded = false;   // nasr_set_step_decode: any bit / bit 1
  bool step_greedy = false;                                              // ... bit 0

  // profiling
  bool profiling = false;
  std::vector<Event> ev_pool;
  size_t ev_used = 0;
  struct Span { int ph; hipEvent_t a, b; };
  std::vector<Span> spans;
  Event ev_total_a, ev_total_b;
  bool window_open = false, total_valid = false;   // timing window [upload|compute_grads .. apply_adam]
  int n_fwd_launch = 0, n_bwd_launch = 0;
  nasr_phase_times last_times;

  // What a handle of the (Bi)LSTM CTC family holds beyond all this (nasr_create); NULL on every other handle.  The last
  // member: the stream session and the family's buffers go before the handle's streams do.
  std::unique_ptr<LstmState, LstmStateDelete> lstm;

  int fail(int code, const std::string& m) {
    t_err = m;
    t_err_handle = this;
    return code;
  }
};

namespace nasr_impl {

#define HIPCHK(h, expr)                                                                                   \
  do {                                                                                                    \
    hipError_t e_ = (expr);                                                                               \
    if (e_ != hipSuccess)                                                                                 \
      return (h)->fail(NASR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                  \
  } while (0)
// the first statement of every model call: a featurizer handle answers NASR_ERR_STATE
#define MODEL_CALL(h)                                                                                     \
  do {                                                                                                    \
    if ((h) && (h)->family == Family::Featurizer)                                                         \
      return (h)->fail(NASR_ERR_STATE, std::string(__func__) + ": a featurizer handle has no model");     \
  } while (0)
// behind it, in the calls that only the (Bi)LSTM families answer: LSTM_CALL(h, "has no dropout")
#define LSTM_CALL(h, reason)                                                                              \
  do {                                                                                                    \
    if ((h) && !(h)->lstm)                                                                                \
      return (h)->fail(NASR_ERR_STATE, std::string(__func__) + ": a WaveNet or LAS handle " reason);      \
  } while (0)
// the first statement of a call that only one family answers: a null handle is NASR_ERR_ARG, a handle of another family
// NASR_ERR_STATE with "<function>: not a LAS handle" / "... not a WaveNet handle"
#define FAMILY_CALL(h, state, text)                                                                       \
  do {                                                                                                    \
    if (!(h)) return NASR_ERR_ARG;                                                                        \
    if (!(h)->state) return (h)->fail(NASR_ERR_STATE, std::string(__func__) + ": " text);                 \
  } while (0)
#define LAS_CALL(h) FAMILY_CALL(h, las, "not a LAS handle")
#define WAVENET_CALL(h) FAMILY_CALL(h, wn, "not a WaveNet handle")
// ---- nasr_api.hip: what the create calls share (a failure leaves its message in g_create_error)
// behind create call fn's own argument checks: a gfx950 device, a new handle on it with the device set and its stream
// (the caller's, or one of its own) in place; prop: the device's properties, or NULL
int handle_open(const char* fn, Family family, int device_id, void* stream, nasr_ctx** out, hipDeviceProp_t* prop);
int create_fail(nasr_ctx* h, int code, const std::string& m);   // destroys the handle
bool alloc_param_buffers(nasr_ctx* h);   // P, M, V, G behind its head, Adam's and the clipping state for np_int floats, zeroed
// once h->buckets is laid out: their events, the copy and logits streams, the batch slots' events, the step-result stamps
// and step-end words, the timing events; then a synchronise.  A failure destroys the handle.
int handle_finish(nasr_ctx* h);

// ---- nasr_layout.hip
int repack(nasr_ctx* h);   // the operand images of an LSTM-family handle's parameters; nothing on any other handle
int scatter_to_device(nasr_ctx* h, const float* tf_flat, float* dev);
int gather_from_device(nasr_ctx* h, const float* dev, float* tf_flat);
// a word in host-mapped pinned memory written in stream order (and, with f0_dst, a device float copied beside it)
void launch_stamp(unsigned* dst, unsigned value, float* f0_dst, const float* f0_src, hipStream_t st);
void launch_publish_results(const float* loss, const float* fault, const int* lens, int Bp, const int* ids, int n_ids, void* host,
                            unsigned* stamp, unsigned value, hipStream_t st);
bool wait_stamp(const uint32_t* w, uint32_t want, double timeout_s);
int sync_checked(nasr_ctx* h);
hipEvent_t next_event(nasr_ctx* h);
struct PhaseScope {
  nasr_ctx* h;
  int ph;
  hipEvent_t a = nullptr;
  PhaseScope(nasr_ctx* h_, int ph_) : h(h_), ph(ph_) {
    if (h->profiling) {
      a = next_event(h);
      (void)hipEventRecord(a, h->st);
    }
  }
  ~PhaseScope() {
    if (h->profiling) {
      hipEvent_t b = next_event(h);
      (void)hipEventRecord(b, h->st);
      h->spans.push_back({ph, a, b});
    }
  }
};

// ---- nasr_rec.hip: what the common calls run on every model handle (nothing where there is no resident recurrence)
int rec_check(nasr_ctx* h);
void rec_rearm(nasr_ctx* h);

// ---- nasr_lstm.hip
// the create-time switches of an LSTM-family handle, as nasr_create read them from the environment (README)
struct LstmSwitches {
  bool compact, persist, rec_f32, wgrad_overlap, bucket_defer;   // NASR_COMPACT, NASR_PERSIST, NASR_REC=f32, NASR_WGRAD_OVERLAP, NASR_BUCKET_DEFER
  int64_t rearm_after;                                            // NASR_PERSIST_REARM
};
// nasr_create behind the reading of the environment: the argument checks, the handle and its LstmState
int lstm_create(const nasr_model_cfg* cfg, int device_id, void* stream, const LstmSwitches& sw, nasr_ctx** out);
// what the common calls run on every model handle (nothing where there is no LstmState)
void drop_graphs(nasr_ctx* h);        // the graphs of the per-step recurrence's layer passes
void lstm_sync_side(nasr_ctx* h);     // waits for the weight-gradient side stream
int lstm_logit_frames(const nasr_ctx* h, int T);   // T: network frames
int lstm_frame_skip(const nasr_ctx* h);             // 1 on a handle of another family

// ---- nasr_batch.hip
// chunked: the batch is laid out in the windows of nasr_set_chunking
int ensure_shape(nasr_ctx* h, int B, int T, int Lmax, bool chunked = false);
// the logits and what the CTC lattice, its loss and the greedy decoder work in (T frames, Tp logit frames); returns the
// lattice kernel's instantiation for labels up to Lmax (h->KS), or the code of a failure (< 0)
int ensure_ctc_buffers(nasr_ctx* h, int B, int Bp, int T, int Tp, int Lmax, bool* grew);
// num_classes: 0 = the handle's (and its family's rules); > 0: CTC labels over that many classes (nasr_ctc_align_logits)
// skip: the CTC feasibility check is made against skip_frames(seq_len[b], skip), the frames the network sees
int validate_batch(nasr_ctx* h, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T, int Lmax,
                   int num_classes = 0, int skip = 1);
// a chunk of a stream session: S slots, Tc frames, n_frames[b] in [0, Tc] (0 = the slot is idle in this chunk)
int validate_chunk(nasr_ctx* h, const int32_t* n_frames, int S, int Tc);
bool pinned_ensure(Pinned<void>& p, size_t* cap, size_t bytes);
void slot_set_state(nasr_ctx* h, BatchSlot* s, int st);
int slot_commit(nasr_ctx* h, BatchSlot* s);
// Where a slot's centre frames and pad values come from when not from host memory: run() enqueues on stream cs whatever
// writes dcentre [B][T][ncep] and dpad [B]; pinned is stage_bytes of the slot's pinned buffer (NULL on a synchronous upload).
struct CentreProducer {
  size_t stage_bytes = 0;
  std::function<int(float* dcentre, float* dpad, void* pinned, hipStream_t cs)> run;
};
// The counterpart for stacked rows: run() enqueues on stream cs whatever writes dfeats [B][T][F], every element of it (a
// stream session's front end: nasr_stream_feed_audio).
struct StackedProducer {
  std::function<int(float* dfeats, hipStream_t cs)> run;
};
// What a batch is, from the ABI entry point to its slot.  Exactly one source: feats (stacked [B][T][F]), centre + pad_value
// (the centre form in host memory: centre frames [B][T][ncep] and one pad value per utterance), producer (the centre
// form, written on the device) or stacked (stacked rows, written on the device).  ctx and ncep (numcontext; the width of one un-stacked frame) mean something in the two
// centre forms only.  labels, label_len and aug are nullable; aug needs a centre form.  Made by the three functions below.
struct BatchSrc {
  const float *feats = nullptr, *centre = nullptr, *pad_value = nullptr;
  const CentreProducer* producer = nullptr;
  const StackedProducer* stacked = nullptr;
  int ctx = 0, ncep = 0;
  const int32_t *seq_len = nullptr, *labels = nullptr, *label_len = nullptr;
  int B = 0, T = 0, Lmax = 0;
  const nasr_batch_aug* aug = nullptr;
  bool chunk = false;   // a chunk of a stream session: seq_len[b] = 0 is an idle slot (validate_chunk instead of validate_batch)
  bool centre_form() const { return centre || producer; }
};
inline BatchSrc stacked_batch(const float* feats, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B,
                              int T, int Lmax) {
  BatchSrc b;
  b.feats = feats; b.seq_len = seq_len; b.labels = labels; b.label_len = label_len; b.B = B; b.T = T; b.Lmax = Lmax;
  return b;
}
inline BatchSrc centre_batch(const float* centre, const float* pad_value, int ctx, int ncep, const int32_t* seq_len,
                             const int32_t* labels, const int32_t* label_len, int B, int T, int Lmax,
                             const nasr_batch_aug* aug) {
  BatchSrc b = stacked_batch(nullptr, seq_len, labels, label_len, B, T, Lmax);
  b.centre = centre; b.pad_value = pad_value; b.ctx = ctx; b.ncep = ncep; b.aug = aug;
  return b;
}
inline BatchSrc produced_batch(const CentreProducer* producer, int ctx, int ncep, const int32_t* seq_len, const int32_t* labels,
                               const int32_t* label_len, int B, int T, int Lmax, const nasr_batch_aug* aug) {
  BatchSrc b = centre_batch(nullptr, nullptr, ctx, ncep, seq_len, labels, label_len, B, T, Lmax, aug);
  b.producer = producer;
  return b;
}
// A batch into a slot (slot_fill: check, lay out the meta block, size the buffers, wait for the slot, write the meta block,
// copy the features, copy the meta block, record ev_copy), then: upload commits it on the compute stream (the synchronous
// upload of nasr_upload_batch / nasr_train_step / ...), stage leaves it STAGED on the copy stream behind *ticket.
int upload(nasr_ctx* h, const BatchSrc& b);
BatchSlot* slot_of_ticket(nasr_ctx* h, int ticket);
int stage(nasr_ctx* h, const BatchSrc& b, int* ticket);

// ---- nasr_pass.hip
// the fp32 GEMM g (gemm.hip) on the handle's stream; g.split_k > 1 gets the handle's slab workspace, grown to fit
int gemm_f32(nasr_ctx* h, GemmDesc g);
// C [M][N] = op(A) op(B) (+ bias per column) as one gemm_f32 call; a_col / b_col: the operand is stored transposed.
// a_shift / a_rows: rows of A are read a_shift rows further on, and rows outside [0, a_rows) read as zero (a_rows < 0: all
// of A, K rows when a_col and M otherwise).  With a bias the product is not split along K.
int gemm_dense(nasr_ctx* h, const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc, bool a_col,
               bool b_col, const float* bias = nullptr, int a_shift = 0, int a_rows = -1);
inline float* fp(const DevBuf& b, size_t off = 0) { return b.as<float>() + off; }
int forward(nasr_ctx* h);   // the CTC logits of the resident batch
// forward pass and loss of the resident batch.  training: the WaveNet's batch norm on the batch's statistics (a LAS
// handle samples either way, one counter value per pass)
int loss_pass(nasr_ctx* h, bool training);
CtcDims ctc_dims(nasr_ctx* h);
int ctc_forward(nasr_ctx* h);
int backward(nasr_ctx* h);
// the distillation term is part of the resident batch's loss and gradient: a weight > 0 and teacher logits for this batch
inline bool distill_on(const nasr_ctx* h) { return h->kd_weight > 0.f && h->resident && h->teach_valid; }
// both CTC families' backward passes start here: the logits, in place, become d(loss)/dlogits - the CTC gradient, and
// with the term on (1 - weight) times it plus what the loss pass left in kd_grad
int logit_grads(nasr_ctx* h);
// rows >= 0: the first `rows` logit frames only
int fetch_logits(nasr_ctx* h, float* logits_out, int rows = -1);

// ---- nasr_wavenet.hip (the WaveNet handle's side of ensure_shape, forward and backward)
int wn_ensure_shape(nasr_ctx* h, int B, int T, int Lmax);
int wn_forward(nasr_ctx* h, bool training);
int wn_backward(nasr_ctx* h);

// ---- nasr_las.hip (the LAS handle's side of ensure_shape, forward and backward; its loss is part of its forward pass)
int las_ensure_shape(nasr_ctx* h, int B, int T, int Lmax);
int las_forward(nasr_ctx* h, bool sample);
int las_backward(nasr_ctx* h);

// ---- nasr_batch.hip, nasr_pass.hip (the LSTM-family handle's side of ensure_shape, forward and backward)
int lstm_ensure_shape(nasr_ctx* h, int B, int T, int Lmax, bool chunked);
// chunk: the resident batch is a chunk of the open stream session - the recurrence continues from the session's state on
// the per-step kernels and saves it again; the fault word, the resident kinds' control blocks and the dropout counter stay
int lstm_forward(nasr_ctx* h, bool chunk = false);
int lstm_backward(nasr_ctx* h);

}  // namespace nasr_impl
