// nasr_ctx.h — what the translation units behind include/nasr.h share: the handle (struct nasr_ctx: model layout, HBM buffers,
// batch slots, streams / events, recurrence mode), small helpers, and the functions they call in each other (internal, C++).
//   nasr_layout.hip  parameter layout, TF <-> internal maps, operand images (repack)
//   nasr_rec.hip     the recurrence's kind: create-time set-up and census, resident launches, abort check, re-arming
//   nasr_batch.hip   batch buffers and slots: upload, stage / commit
//   nasr_pass.hip    forward, CTC, backward: the orchestration of one step on the handle's streams
//   nasr_stream.hip  streaming sessions (nasr_stream_*): recurrent state that survives between chunks
//   nasr_api.hip     the C ABI entry points; what the create calls share (handle_open, alloc_param_buffers, handle_finish)
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
#include <map>
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

struct GraphKey {
  int T, l, bwd;
  bool operator<(const GraphKey& o) const {
    if (T != o.T) return T < o.T;
    if (l != o.l) return l < o.l;
    return bwd < o.bwd;
  }
};

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

// the kinds of kernels that run the recurrence; the values are the codes of nasr_get_recurrence_mode
enum class RecKind { Step = 0, Persist = 1, Wide = 2 };

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

// The front end of a stream session that takes samples (nasr_fz.hip: nasr_stream_attach_audio); NULL while the session is
// fed finished frames.
struct FzStream;
struct FzStreamDelete { void operator()(FzStream* f) const; };

// A stream session (nasr_stream.hip): S concurrent streams with a look-ahead of R frames.  R = 0 on a unidirectional
// LSTM-family handle (nasr_stream_open: nothing is ever held), R >= 1 on a bidirectional one whose backward direction
// restarts in every window (nasr_stream_open_lookahead).
struct StreamState {
  int S = 0;
  int R = 0;                         // look-ahead frames
  std::unique_ptr<FzStream, FzStreamDelete> audio;   // per slot: sample tail, running sums, waiting and recent frames
  DevBuf state;                      // [L][S][2][H] fp32: c, then h, as of each slot's last (emitted) frame; zero after open / reset
  DevBuf cimg;                       // [D][Bp][Hp]: the layer's saved c as step 0 of a feed reads it
  DevBuf hold[2];                    // R > 0: [S][R][F] held feature rows; a feed reads hold[cur] and writes the other one
  int cur = 0;
  DevBuf fresh;                      // R > 0: [S][Tc][F] the feed's new rows: uploaded, or made by the front end
  std::vector<int32_t> held;         // [S] rows held
  std::vector<uint8_t> done;         // [S] the slot has had `last` and no reset
  LaSlots sl{};                      // the feed that is running (run_chunk_steps: which row's state to save)
  std::vector<int64_t> frames;       // [S] frames emitted since the slot's reset
};

}  // namespace nasr_impl

// (internal header: the translation units behind the ABI use both namespaces unqualified)
using namespace nasr;
using namespace nasr_impl;

struct nasr_ctx {

  nasr_model_cfg cfg;
  Family family = Family::Lstm;
  std::unique_ptr<WnState, WnStateDelete> wn;   // a WaveNet handle (nasr_create_wavenet); the LSTM members stay unused
  std::unique_ptr<FzState, FzStateDelete> fz;   // a featurizer handle (nasr_create_featurizer): no model at all
  std::unique_ptr<LasState, LasStateDelete> las;   // a LAS handle (nasr_create_las); the LSTM members stay unused
  int device = 0;
  Stream st;
  // Bulk GEMMs (input projections, input / weight gradients, dense stages): fp32 products from two fp16 planes per
  // operand and three MFMA products (gemm_tph.hip); the planes are tiled copies made once per operand.
  DevPtr<unsigned char> WfTP;          // per layer planes of Wx^T [D*N4][Ip]: B operand of the input GEMM
  DevPtr<unsigned char> WbTP;          // per layer (l >= 1) planes of Wx [Ip][D*N4]: B operand of the input-gradient GEMM
  std::vector<size_t> off_wftp, off_wbtp;
  // The recurrence (nasr_rec.hip): the per-step kernels (lstm.hip, one launch per timestep), the persistent kernels for
  // Hp <= 512 (lstm_persist.hip, one launch per layer pass) or the wide ones for Hp = 2048 (lstm_wide.hip, one launch per
  // direction and pass).  The resident kinds need the full 8 XCD x 32 CU chip; NASR_PERSIST=0 keeps the per-step kernels.
  RecKind rec_kind = RecKind::Step;    // kind: the resident kind set up at create (Step: none, or the census failed)
  RecKind rec_use = RecKind::Step;     // in use: Step or the kind (nasr_get_recurrence_mode)
  bool rec_wanted = false;             // wanted: the kind is what this handle should run when the device allows it
  bool rec_inflight = false;           // inflight: a resident launch has run since *perr was last checked
  bool rec_refused = false;            // refused until re-armed: an abort sets it; the persistent kind refuses set(1) meanwhile
  // re-arming after an abort (rec_check): `rearm_after` clean steps on the per-step kernels, then back to the kind (rec_rearm);
  // every further abort doubles the wait.  NASR_PERSIST_REARM sets the first wait (0 = never re-arm).
  int64_t rearm_after = 0, rearm_wait = 0, clean_steps = 0;
  int persist_aborts = 0, persist_rearms = 0;
  uint64_t repack_seq = 0;             // counts repack(): the parameters' operand images changed
  uint64_t step_img_seq = ~0ull;       // repack_seq of the per-step operand images Uf / Ub (ensure_step_images)
  std::unique_ptr<StreamState> stream; // the open stream session, or none
  Pinned<unsigned> perr;               // host-mapped sticky error word of the resident launches
  DevPtr<float> Ucs, Ucinv;            // [L*D][N4] column scales / inverse scales of every (layer, direction) recurrent matrix
  // the persistent kind: [L][D] operand images; the forward recurrence on fp16 planes of U (v_mfma_f32_4x4x4_16B_f16)
  // under the column scales Ucs, measured after every optimiser step.  NASR_REC=f32 keeps fp32 MFMAs.
  bool rec_f16 = false;
  DevPtr<float> Upf, Upb;
  size_t imf = 0, imb = 0;             // floats per (layer, direction) image
  // the hand-offs validate themselves by epoch bits (lstm_persist.hip) and start from cleared buffers: one buffer per
  // layer pass, all of a pass cleared in one go
  DevPtr<float> xchf;                  // [L] h exchange buffers of the forward launches (persist_hx_bytes each)
  DevPtr<float> xchb;                  // [L] partial-sum exchange buffers of the BPTT launches (persist_px_bytes each)
  DevPtr<PersistCtl> pctl;
  // the wide kind: U resident in the registers of all 256 CUs, forward and BPTT
  DevPtr<unsigned char> Uw;            // [L][D] forward operand images (wide_image_bytes each) under the column scales Ucs
  DevPtr<unsigned char> Uwb;           // [L][D] BPTT operand images (U^T fragments under per-row scales)
  DevPtr<float> Urs, Urinv;            // [L*D][Hp] row scales of every recurrent matrix and their inverses
  DevPtr<float> wsrow;                 // [D][64] dG scale per (direction, utterance) of the running BPTT pass
  DevPtr<void> whx;                    // h exchange
  DevPtr<float> wpart;                 // cross-XCD inboxes: partial sums (forward) / dG planes (BPTT)
  DevPtr<void> wpx;                    // BPTT: partial dh through the XCD's L2
  DevPtr<WideCtl> wctl;
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

  // model dims
  int F, Fp, H, Hp, N4, D, L, C, Cp, Pin, Pinp;
  std::vector<int> Ip;                  // padded input width per layer
  std::vector<int64_t> off_wx, off_bias;  // per layer
  std::vector<int64_t> off_u;           // per (layer, dir)
  int64_t off_w = 0, off_b = 0, np_int = 0;
  std::vector<TensorInfo> tensors;
  int64_t np_tf = 0;
  std::vector<int32_t> tf2int;          // TF flat index -> internal flat index

  // dense stages of the DeepSpeech family (networks/deepspeech.py): stage i < npre feeds the LSTM stack, stage npre
  // (when has_post) sits between the stack and the logits.  W_i [dIp][dWp] row-major, b_i [dWp].
  int npre = 0, ndense = 0;
  bool has_post = false;
  int F0 = 0;                            // unpadded input width of LSTM layer 0 (F, or the last pre stage's width)
  std::vector<int> dWid, dWp, dIn, dIp;
  std::vector<int64_t> off_dw, off_db;
  std::vector<size_t> off_dftp, off_dbtp;
  DevPtr<unsigned char> DfTP, DbTP;      // TP of W_i^T [dWp][dIp] and of W_i [dIp][dWp]
  std::vector<DevBuf> Ybuf, dYbuf;       // stage outputs and their gradients [R][dWp]
  DevBuf DTP;                            // scratch: TP of a stage input with the frame index as contraction index
  uint32_t drop_seed = 4567u, drop_counter = 0;   // random_seed of networks/deepspeech.py:26

  DevPtr<float> P, M, V, Uf, Ub;
  float* G = nullptr;                        // Gbase + GRAD_HEAD
  // Every operand row of a plane GEMM carries a power-of-two scale (device floats, scale and 1/scale), measured per step
  // for everything whose range is not known in advance.
  struct SV {
    DevBuf s, inv;
    bool ensure(size_t n) { bool g = false; return s.ensure(n * 4, &g) && inv.ensure(n * 4, &g); }
    float* sp() const { return s.as<float>(); }
    float* ip() const { return inv.as<float>(); }
  };
  SV sc15;                                   // constants 2^15 / 2^-15: LSTM outputs (|h| < 1), rows and columns
  size_t sc15_n = 0;
  SV sc_x0r, sc_x0c;                         // features: per frame row / per feature column
  std::vector<SV> sc_yr, sc_yc;              // dense stage outputs
  SV sc_gr, sc_gc;                           // the gate / dense pre-activation gradient being worked on
  std::vector<SV> sc_wr, sc_wc;              // Wx[l]: per input row / per gate column
  std::vector<SV> sc_dr, sc_dc;              // dense W[i]
  DevBuf scws;                               // partial maxima (launch_tph_scales)
  int gttp_layer = -1;                       // layer whose transposed dG planes gemm_dx has just written (fused split)
  int dgmax_layer = -1;                      // layer whose |dG| maxima the persistent BPTT kernel has left in `dgmax`
  DevBuf dgmax;                              // [D*32][R] row parts | [8/D][D*N4] column parts (persist_dgmax_floats)
  DevPtr<float> Gbase;                       // allocation behind G: [GRAD_HEAD floats, [0] = fault word][np_int gradients]
  // gradient buckets: (offset, count) in floats from Gbase, in the order backward() completes them; one event each
  std::vector<std::pair<int64_t, int64_t>> buckets;
  std::vector<Event> ev_bucket;
  std::vector<int> bucket_of_layer;          // LSTM layer -> bucket whose last gradients are that layer's (-1: none)
  // Persistent mode: bucket(l)'s event is recorded AFTER the persistent BPTT launch of layer l-1 instead of right after
  // weight_grads(l), so that a collective released by it co-runs with the GEMM phase of layer l-1, not with the launch
  // that wants every CU's memory queue to itself (nasr_set_bucket_defer; NASR_BUCKET_DEFER=0 at create).
  bool bucket_defer = true;
  // Adam's step count t lives ON THE DEVICE (AdamDev, optim.hip): the launch that finds the step's fault word set leaves
  // it alone, so a void step never enters the bias correction - whenever the host learns about it.
  DevPtr<AdamDev> adam_dev;
  float lr;
  // Global-norm gradient clipping (nasr_set_grad_clip; 0 = off, the default: nasr_apply_adam then launches what it always
  // did).  The norm, the decision and the counters live on the device beside AdamDev, so the step stays asynchronous.
  float max_grad_norm = 0.f;
  DevPtr<ClipDev> clip_dev;
  DevPtr<double> clip_part;                  // GRAD_SUMSQ_MAX_BLOCKS partial sums of squares
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
  int B = 0, Bp = 0, T = 0, Lmax = 0, Tp = 0, KS = 1;
  // Latency-controlled training (nasr_set_chunking): lcC > 0 = every whole-batch pass runs the utterances'
  // windows of lcC + lcR rows.  The LSTM stack then works on a virtual time axis of Tv = K*W rows (kernels.h, LcGeom) - its
  // activations, planes and gradients are sized and indexed by Tv, always through the compacted-row lists (cmp_rows: the
  // rows the windows have; vprev / vnext stop at a window's edges, vprev of a window's first row is the row the forward
  // state was carried from) - while the projection and the CTC stay on the T frames: lc_top / lc_dtop hold the top layer's
  // emitted rows and their gradient by frame.  Tv = T and lc_live = false for every other batch (a stream chunk included).
  int lcC = 0, lcR = 0;
  int Tv = 0;
  bool lc_live = false;                      // the resident batch is laid out in windows
  LcGeom lcg{};
  int32_t* wlen_p = nullptr;                 // [K][Bp] rows of every window (inside cur->dmeta)
  DevBuf lc_x0, lc_top, lc_dtop;             // features by frame [T*Bp][Fp]; top layer's emitted rows / their gradient [T*Bp][Pinp]
  DevBuf lc_cimg, lc_dcc;                    // the carried c of the window being run [D][Bp][Hp]; carried dc [Bp][Hp]
  int64_t frames = 0;
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
  // the recurrent weight gradient).  cmp_rows = Rv (0: no compaction for the resident batch).  NASR_COMPACT=0 turns it off.
  bool compactable = false;
  int cmp_rows = 0, cmp_rows_p = 0;
  int32_t *vrow_p = nullptr, *vprev_p = nullptr, *vnext_p = nullptr;
  SV sc_cr, sc_cx;                           // row scales gathered to the compacted order: dG rows / feature rows
  DevBuf OTS;                                // planes of shift(out[l])^T over the compacted rows (recurrent weight gradient)

  // Weight gradients under the BPTT of the layer below (persistent mode, Hp = 512, L > 1; NASR_WGRAD_OVERLAP=0 turns it off): weight_grads(l)
  // runs on a low-priority side stream in the 3-wave GEMM instantiation that fits on a CU beside a persistent workgroup,
  // from its own copies of everything the main stream rewrites meanwhile (dG^T planes, column scales, partial column sums,
  // slabs: index l & 1), and is joined before layer l's gradients are released / Adam.
  bool wg_overlap = false;
  bool bwd_lean = false;                     // the side stream exists: persistent BPTT launches leave it room (launch_lstm_persist_bwd)
  Stream wst;
  Event ev_dx;
  std::vector<Event> ev_wg;                  // per layer: its weight gradients are complete
  std::vector<char> wg_pending;              // ... and the main stream has not waited for that yet
  DevBuf GTTP2, csws2, slabs2;
  SV sc_gc2;
  DevBuf XTP, X0TTP, GTP, GTTP;   // tiled-plane copies of activations / dG
  std::vector<DevBuf> OTT;        // per layer: planes of out[l] with the frame index as contraction index (weight gradients)
  std::vector<char> ott_valid;    // ... written by the forward pass of this step already (together with the planes of layer l+1's input)
  DevBuf ctcprobs, ctckexp;                  // emission rows and column offsets of the CTC lattice (ctc.hip (2b))
  DevBuf seqbuf, X0, logits, logz, alpha, beta, aoff, boff, logp, nll, loss, slabs, csws, amax, ids, lens,
      stage;
  // forced alignment (nasr_ctc_align*): workspaces of its own, sized at the first call that needs them - its logZ rows, the
  // back-pointers that do not fit in LDS, path and score; and for nasr_ctc_align_logits the caller's logits and labels
  DevBuf al_logz, al_bp, al_path, al_score, al_logits, al_meta;
  std::vector<DevBuf> gates, outb, cbuf;
  DevBuf dout, hstate, partial, dcstate, dgbuf;   // shared by the layers (a layer's backward pass is over before the next starts)

  // graphs
  bool graph_mode = true;
  bool step_decode = false, step_logits = false, have_decoded = false;   // nasr_set_step_decode: any bit / bit 1
  bool step_greedy = false;                                              // ... bit 0
  std::map<GraphKey, hipGraphExec_t> graphs;

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
    if ((h) && (h)->family != Family::Lstm)                                                               \
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
// ---- tiled fp16 planes (gemm_tph.hip) ---------------------------------------------------------------------------
inline size_t pl_rb_bytes(int nkb) { return (size_t)nkb * 2 * 1024; }   // one 32-row block: nkb k-blocks x 2 parts x 1 KiB
// scales of src [rows][K]: per row into `row`, per column into `col` (either may be NULL)
void pl_scales(nasr_ctx* h, const float* src, int rows, int K, int ld, nasr_ctx::SV* row, nasr_ctx::SV* col, hipStream_t st);
// planes of src [rows][K] (tpN, scaled per row by rs[]) and / or of its transpose (tpT, scaled per src column by cs[]);
// colpart: 64-row partial column sums for launch_colsum_parts
void pl_split(const float* src, unsigned char* tpN, unsigned char* tpT, int rows, int K, int ld, const float* rs,
              const float* cs, float* colpart, hipStream_t st);
// a_inv / b_inv: inverse scales of A's / B's rows; the strides apply to batch 1 of a two-batch launch
void pl_gemm(GemmTPHDesc g, const float* a_inv, const float* b_inv, hipStream_t st, int64_t ainv_bstride = 0,
             int64_t binv_bstride = 0);
// scale vectors of an activation tensor: the features, a dense stage's output (index i), or an LSTM layer's output
struct ActScale { const float *rs, *rinv, *cs, *cinv; };
inline ActScale act_x0(const nasr_ctx* h) { return {h->sc_x0r.sp(), h->sc_x0r.ip(), h->sc_x0c.sp(), h->sc_x0c.ip()}; }
inline ActScale act_y(const nasr_ctx* h, int i) { return {h->sc_yr[i].sp(), h->sc_yr[i].ip(), h->sc_yc[i].sp(), h->sc_yc[i].ip()}; }
inline ActScale act_out(const nasr_ctx* h) { return {h->sc15.sp(), h->sc15.ip(), h->sc15.sp(), h->sc15.ip()}; }
inline ActScale lstm_in_scale(const nasr_ctx* h, int l) {
  if (l > 0) return act_out(h);
  return h->npre ? act_y(h, h->npre - 1) : act_x0(h);
}
inline ActScale dense_in_scale(const nasr_ctx* h, int i) {
  if (i == 0 && h->npre > 0) return act_x0(h);
  if (i < h->npre) return act_y(h, i - 1);
  return act_out(h);                               // the post stage reads the top LSTM layer
}

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
int build_layout(nasr_ctx* h);
int repack(nasr_ctx* h);
int scatter_to_device(nasr_ctx* h, const float* tf_flat, float* dev);
int gather_from_device(nasr_ctx* h, const float* dev, float* tf_flat);
// a word in host-mapped pinned memory written in stream order (and, with f0_dst, a device float copied beside it)
void launch_stamp(unsigned* dst, unsigned value, float* f0_dst, const float* f0_src, hipStream_t st);
void launch_publish_results(const float* loss, const float* fault, const int* lens, int Bp, const int* ids, int n_ids, void* host,
                            unsigned* stamp, unsigned value, hipStream_t st);
bool wait_stamp(const uint32_t* w, uint32_t want, double timeout_s);
int sync_checked(nasr_ctx* h);
void drop_graphs(nasr_ctx* h);
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

// ---- nasr_rec.hip
int rec_setup(nasr_ctx* h, bool allowed, bool f32);   // allowed: NASR_PERSIST is not 0 and the chip is whole; f32: NASR_REC=f32
void rec_start(nasr_ctx* h);                          // the census, once the handle's streams exist
int rec_launch(nasr_ctx* h, int l, bool bwd, hipStream_t st, int* launches);
int rec_check(nasr_ctx* h);
void rec_rearm(nasr_ctx* h);
std::vector<TphScaleJob> rec_scale_jobs(const nasr_ctx* h);   // repack: scale jobs, then images of the recurrent matrices
void rec_images(nasr_ctx* h);
// repack() keeps the per-step operand images Uf / Ub only while the per-step kernels run the handle's batches.  A stream feed
// and a chunked pass need them whatever the kind: rebuilt here iff a resident kind is in use and they are older than repack_seq.
void ensure_step_images(nasr_ctx* h);

// ---- nasr_batch.hip
// chunked: the batch is laid out in the windows of nasr_set_chunking (h->lcC, h->lcR)
int ensure_shape(nasr_ctx* h, int B, int T, int Lmax, bool chunked = false);
// the logits and what the CTC lattice, its loss and the greedy decoder work in (T frames, Tp logit frames); returns the
// lattice kernel's instantiation for labels up to Lmax (h->KS), or the code of a failure (< 0)
int ensure_ctc_buffers(nasr_ctx* h, int B, int Bp, int T, int Tp, int Lmax, bool* grew);
// num_classes: 0 = the handle's (and its family's rules); > 0: CTC labels over that many classes (nasr_ctc_align_logits)
int validate_batch(nasr_ctx* h, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T, int Lmax,
                   int num_classes = 0);
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

inline float* dout_of(nasr_ctx* h, int) { return h->dout.as<float>(); }
inline float* dg_of(nasr_ctx* h, int) { return h->dgbuf.as<float>(); }
// what weight_grads(l) reads of layer l's dG: with the overlap on, odd layers have copies of their own (the main stream
// is rewriting the others for layer l-1 while the side stream still reads these)
inline bool wg_alt(const nasr_ctx* h, int l) { return h->wg_overlap && (l & 1); }
inline unsigned char* gttp_of(nasr_ctx* h, int l) { return (wg_alt(h, l) ? h->GTTP2 : h->GTTP).as<unsigned char>(); }
inline float* csws_of(nasr_ctx* h, int l) { return (wg_alt(h, l) ? h->csws2 : h->csws).as<float>(); }
inline nasr_ctx::SV& gc_of(nasr_ctx* h, int l) { return wg_alt(h, l) ? h->sc_gc2 : h->sc_gc; }
// input of LSTM layer l: the features, the last pre-dense stage's output, or the layer below
inline const float* lstm_input(nasr_ctx* h, int l) {
  if (l > 0) return h->outb[l - 1].as<float>();
  return h->npre ? h->Ybuf[h->npre - 1].as<float>() : h->X0.as<float>();
}

// ---- nasr_pass.hip
// the fp32 GEMM g (gemm.hip) on the handle's stream; g.split_k > 1 gets the handle's slab workspace, grown to fit
int gemm_f32(nasr_ctx* h, GemmDesc g);
// C [M][N] = op(A) op(B) (+ bias per column) as one gemm_f32 call; a_col / b_col: the operand is stored transposed.
// a_shift / a_rows: rows of A are read a_shift rows further on, and rows outside [0, a_rows) read as zero (a_rows < 0: all
// of A, K rows when a_col and M otherwise).  With a bias the product is not split along K.
int gemm_dense(nasr_ctx* h, const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc, bool a_col,
               bool b_col, const float* bias = nullptr, int a_shift = 0, int a_rows = -1);
inline float* fp(const DevBuf& b, size_t off = 0) { return b.as<float>() + off; }
// chunk: the resident batch is a chunk of the open stream session - the recurrence continues from the session's state on
// the per-step kernels and saves it again; the fault word, the resident kinds' control blocks and the dropout counter stay
int forward(nasr_ctx* h, bool chunk = false);
// One layer pass of the recurrence over the resident batch's windows (h->lc_live), on the per-step kernels whatever kind
// the handle runs: forward window by window, each from the state carried out of the one before; BPTT in reverse order,
// the carried state's gradient handed back to the window it came from.
int lc_run_steps(nasr_ctx* h, int l, bool bwd, hipStream_t st, int* launches);
// forward pass and loss of the resident batch.  training: the WaveNet's batch norm on the batch's statistics (a LAS
// handle samples either way, one counter value per pass)
int loss_pass(nasr_ctx* h, bool training);
CtcDims ctc_dims(nasr_ctx* h);
int ctc_forward(nasr_ctx* h);
int backward(nasr_ctx* h);
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

}  // namespace nasr_impl
