// nasr_lstm.h — what a handle of the (Bi)LSTM CTC family holds beyond the common parts of nasr_ctx.h (struct LstmState:
// model dimensions, operand images and scales, the recurrence's kind, the weight-gradient side stream, chunked training, the
// stream session, the dense stages, the per-layer activations), and the functions that work on it.  Included only by the
// translation units that run on such a handle: the LSTM side of nasr_layout.hip, nasr_batch.hip and nasr_pass.hip,
// nasr_rec.hip, nasr_stream.hip and nasr_lstm.hip.  The rule: a member lives in nasr_ctx if and only if code that runs on a
// handle of another family reads or writes it.
#pragma once
#include "nasr_ctx.h"

#include <map>

namespace nasr_impl {

// the kinds of kernels that run the recurrence; the values are the codes of nasr_get_recurrence_mode
enum class RecKind { Step = 0, Persist = 1, Wide = 2 };

struct GraphKey {
  int T, l, bwd;
  bool operator<(const GraphKey& o) const {
    if (T != o.T) return T < o.T;
    if (l != o.l) return l < o.l;
    return bwd < o.bwd;
  }
};

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
  // Frame skip: the input rows the slot's utterance has had so far, modulo the skip.  A feed keeps the new
  // rows whose index in the utterance is a multiple of the skip; everything above counts kept rows.
  std::vector<int32_t> phase;        // [S]
  DevBuf raw;                        // skip > 1: [S][Tc][F] the feed's new input rows, before skip_rows_kernel
};

// Every operand row of a plane GEMM carries a power-of-two scale (device floats, scale and 1/scale), measured per step
// for everything whose range is not known in advance.
struct SV {
  DevBuf s, inv;
  bool ensure(size_t n) { bool g = false; return s.ensure(n * 4, &g) && inv.ensure(n * 4, &g); }
  float* sp() const { return s.as<float>(); }
  float* ip() const { return inv.as<float>(); }
};

struct LstmState {
  nasr_model_cfg cfg;                  // as nasr_create took it (merge = NONE on a unidirectional network)

  // model dims (F, Fp, C, Cp: nasr_ctx)
  int H, Hp, N4, D, L, Pin, Pinp;
  std::vector<int> Ip;                  // padded input width per layer
  std::vector<int64_t> off_wx, off_bias;  // per layer
  std::vector<int64_t> off_u;           // per (layer, dir)
  int64_t off_w = 0, off_b = 0;

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

  // Bulk GEMMs (input projections, input / weight gradients, dense stages): fp32 products from two fp16 planes per
  // operand and three MFMA products (gemm_tph.hip); the planes are tiled copies made once per operand.
  DevPtr<unsigned char> WfTP;          // per layer planes of Wx^T [D*N4][Ip]: B operand of the input GEMM
  DevPtr<unsigned char> WbTP;          // per layer (l >= 1) planes of Wx [Ip][D*N4]: B operand of the input-gradient GEMM
  std::vector<size_t> off_wftp, off_wbtp;
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
  DevBuf XTP, X0TTP, GTP, GTTP;   // tiled-plane copies of activations / dG
  std::vector<DevBuf> OTT;        // per layer: planes of out[l] with the frame index as contraction index (weight gradients)
  std::vector<char> ott_valid;    // ... written by the forward pass of this step already (together with the planes of layer l+1's input)
  DevBuf csws;                    // column-sum partials (bias gradients: of the projection too, in this family's backward pass)

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
  DevPtr<float> Uf, Ub;                // the per-step kernels' images of every recurrent matrix
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
  // the per-step kernels' launches of a layer pass, replayed from a hipGraph (run_steps; only this family's pass has any)
  std::map<GraphKey, hipGraphExec_t> graphs;

  std::unique_ptr<StreamState> stream; // the open stream session, or none

  std::vector<int> bucket_of_layer;          // LSTM layer -> bucket whose last gradients are that layer's (-1: none)
  // Persistent mode: bucket(l)'s event is recorded AFTER the persistent BPTT launch of layer l-1 instead of right after
  // weight_grads(l), so that a collective released by it co-runs with the GEMM phase of layer l-1, not with the launch
  // that wants every CU's memory queue to itself (nasr_set_bucket_defer; NASR_BUCKET_DEFER=0 at create).
  bool bucket_defer = true;

  // Latency-controlled training (nasr_set_chunking): lcC > 0 = every whole-batch pass runs the utterances'
  // windows of lcC + lcR rows.  The LSTM stack then works on a virtual time axis of Tv = K*W rows (kernels.h, LcGeom) - its
  // activations, planes and gradients are sized and indexed by Tv, always through the compacted-row lists (cmp_rows: the
  // rows the windows have; vprev / vnext stop at a window's edges, vprev of a window's first row is the row the forward
  // state was carried from) - while the projection and the CTC stay on the T frames: lc_top / lc_dtop hold the top layer's
  // emitted rows and their gradient by frame.  Tv = T and lc_live = false for every other batch (a stream chunk included).
  int lcC = 0, lcR = 0;
  // Frame skip (nasr_set_frame_skip): the network sees input frames 0, skip, 2*skip, ... of every utterance.
  // Only the batch funnel's layout (nasr_batch.hip) and a stream session's row source (nasr_stream.hip) read it.
  int skip = 1;
  int Tv = 0;
  bool lc_live = false;                      // the resident batch is laid out in windows
  LcGeom lcg{};
  DevBuf lc_x0, lc_top, lc_dtop;             // features by frame [T*Bp][Fp]; top layer's emitted rows / their gradient [T*Bp][Pinp]
  DevBuf lc_cimg, lc_dcc;                    // the carried c of the window being run [D][Bp][Hp]; carried dc [Bp][Hp]

  // Ragged batches (nasr_ctx: cmp_rows and the row lists of the resident batch): whether this handle compacts them at all
  // (a plain (Bi)LSTM stack; NASR_COMPACT=0 and nasr_set_row_compaction turn it off), and what only the compacted passes use
  bool compactable = false;
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

  std::vector<DevBuf> gates, outb, cbuf;
  DevBuf dout, hstate, partial, dcstate, dgbuf;   // shared by the layers (a layer's backward pass is over before the next starts)
};

// ---- tiled fp16 planes (gemm_tph.hip) ---------------------------------------------------------------------------
inline size_t pl_rb_bytes(int nkb) { return (size_t)nkb * 2 * 1024; }   // one 32-row block: nkb k-blocks x 2 parts x 1 KiB
// scales of src [rows][K]: per row into `row`, per column into `col` (either may be NULL)
void pl_scales(nasr_ctx* h, const float* src, int rows, int K, int ld, SV* row, SV* col, hipStream_t st);
// planes of src [rows][K] (tpN, scaled per row by rs[]) and / or of its transpose (tpT, scaled per src column by cs[]);
// colpart: 64-row partial column sums for launch_colsum_parts
void pl_split(const float* src, unsigned char* tpN, unsigned char* tpT, int rows, int K, int ld, const float* rs,
              const float* cs, float* colpart, hipStream_t st);
// a_inv / b_inv: inverse scales of A's / B's rows; the strides apply to batch 1 of a two-batch launch
void pl_gemm(GemmTPHDesc g, const float* a_inv, const float* b_inv, hipStream_t st, int64_t ainv_bstride = 0,
             int64_t binv_bstride = 0);
// scale vectors of an activation tensor: the features, a dense stage's output (index i), or an LSTM layer's output
struct ActScale { const float *rs, *rinv, *cs, *cinv; };
inline ActScale act_x0(const LstmState* ls) { return {ls->sc_x0r.sp(), ls->sc_x0r.ip(), ls->sc_x0c.sp(), ls->sc_x0c.ip()}; }
inline ActScale act_y(const LstmState* ls, int i) { return {ls->sc_yr[i].sp(), ls->sc_yr[i].ip(), ls->sc_yc[i].sp(), ls->sc_yc[i].ip()}; }
inline ActScale act_out(const LstmState* ls) { return {ls->sc15.sp(), ls->sc15.ip(), ls->sc15.sp(), ls->sc15.ip()}; }
inline ActScale lstm_in_scale(const LstmState* ls, int l) {
  if (l > 0) return act_out(ls);
  return ls->npre ? act_y(ls, ls->npre - 1) : act_x0(ls);
}
inline ActScale dense_in_scale(const LstmState* ls, int i) {
  if (i == 0 && ls->npre > 0) return act_x0(ls);
  if (i < ls->npre) return act_y(ls, i - 1);
  return act_out(ls);                               // the post stage reads the top LSTM layer
}

// ---- nasr_layout.hip
int build_layout(nasr_ctx* h);

// ---- nasr_rec.hip (rec_check, rec_rearm: nasr_ctx.h)
int rec_setup(nasr_ctx* h, bool allowed, bool f32);   // allowed: NASR_PERSIST is not 0 and the chip is whole; f32: NASR_REC=f32
void rec_start(nasr_ctx* h);                          // the census, once the handle's streams exist
int rec_launch(nasr_ctx* h, int l, bool bwd, hipStream_t st, int* launches);
std::vector<TphScaleJob> rec_scale_jobs(const nasr_ctx* h);   // repack: scale jobs, then images of the recurrent matrices
void rec_images(nasr_ctx* h);
// repack() keeps the per-step operand images Uf / Ub only while the per-step kernels run the handle's batches.  A stream feed
// and a chunked pass need them whatever the kind: rebuilt here iff a resident kind is in use and they are older than repack_seq.
void ensure_step_images(nasr_ctx* h);

inline float* dout_of(LstmState* ls, int) { return ls->dout.as<float>(); }
inline float* dg_of(LstmState* ls, int) { return ls->dgbuf.as<float>(); }
// what weight_grads(l) reads of layer l's dG: with the overlap on, odd layers have copies of their own (the main stream
// is rewriting the others for layer l-1 while the side stream still reads these)
inline bool wg_alt(const LstmState* ls, int l) { return ls->wg_overlap && (l & 1); }
inline unsigned char* gttp_of(LstmState* ls, int l) { return (wg_alt(ls, l) ? ls->GTTP2 : ls->GTTP).as<unsigned char>(); }
inline float* csws_of(LstmState* ls, int l) { return (wg_alt(ls, l) ? ls->csws2 : ls->csws).as<float>(); }
inline SV& gc_of(LstmState* ls, int l) { return wg_alt(ls, l) ? ls->sc_gc2 : ls->sc_gc; }
// input of LSTM layer l: the features, the last pre-dense stage's output, or the layer below
inline const float* lstm_input(nasr_ctx* h, int l) {
  LstmState* ls = h->lstm.get();
  if (l > 0) return ls->outb[l - 1].as<float>();
  return ls->npre ? ls->Ybuf[ls->npre - 1].as<float>() : h->X0.as<float>();
}

// ---- nasr_pass.hip
// One layer pass of the recurrence over the resident batch's windows (lc_live), on the per-step kernels whatever kind
// the handle runs: forward window by window, each from the state carried out of the one before; BPTT in reverse order,
// the carried state's gradient handed back to the window it came from.
int lc_run_steps(nasr_ctx* h, int l, bool bwd, hipStream_t st, int* launches);

}  // namespace nasr_impl
