// kernels.h — launch wrappers of the gfx950 kernels behind libnasr.so (internal, C++).
// Data layout in HBM (all fp32, time-major, padded):
//   rows   r = t*Bp + b           Bp = round_up(B,16)
//   X0     [R][Fp]                Fp = round_up(F,32)
//   gates  [R][D*N4]              N4 = 4*Hp, Hp = round_up(H,64); column d*N4 + 4*j + g (gate-interleaved)
//   out,c  [R][D*Hp]
//   logits [T'*Bp][Cp]            Cp = round_up(C,32)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace nasr {

// Fault-injection hooks of the tests (NASR_PERSIST_FAULT, NASR_WIDE_FAULT, ...): honoured only in a process that had
// NASR_TEST_HOOKS=1 in its environment when the library first asked - a stray variable in a production run does nothing,
// and a production launch costs one cached bool instead of getenv calls.
const char* test_hook(const char* name);

// ---- GEMM (gemm.hip): C[M,N] = opA[M,K] * opB[K,N] (+bias[n]) on v_mfma_f32_32x32x2_f32 ----
struct GemmDesc {
  const float* A;
  const float* B;
  float* C;
  int M, N, K;          // K % 4 == 0, M % 4 == 0, N % 4 == 0
  int lda, ldb, ldc;    // element strides (multiples of 4)
  bool a_col;           // false: A(m,k) = A[row(m)*lda + k]      true: A(m,k) = A[row(k)*lda + m]
  bool b_col;           // false: B(k,n) = B[k*ldb + n]           true: B(k,n) = B[n*ldb + k]
  const int* a_map;     // logical->physical row of A (-1 = zero row); NULL: physical = logical + a_shift
  int a_shift;          // row shift applied when a_map == NULL
  int a_rows;           // physical rows of A (rows outside [0,a_rows) read as zero)
  const int* c_map;     // logical->physical row of C (-1 = skip); NULL: identity
  const float* bias;    // per-n bias or NULL
  int split_k;          // >=1; >1 writes partial slabs to `slabs` and reduces them into C
  float* slabs;         // workspace of split_k*M*N floats (only when split_k > 1)
};
void launch_gemm(const GemmDesc& g, hipStream_t st);
int gemm_pick_split(int M, int N, int K);

// ---- fp32-accurate GEMM from pre-split, pre-tiled fp16 operands (gemm_tph.hip): C[M,N] = A[M,K] * B[N,K]^T (+bias) ----
// A "tiled planes" operand holds the two fp16 parts of a scaled fp32 matrix [rows][K] as 1 KiB tiles
// TPH[row/32][k/16][part][32 rows x 16 k]; tph_bytes() sizes it, launch_tph_split2() fills it from fp32.
int tp_split2_parts(int rows);           // 64-row partial column sums the split pass can emit
int gemm_tp_tile_rows(int M);            // 256, or 192 where 256-row tiles would leave > 10 % of their rows empty
// Every operand row carries a power-of-two scale (constant along the contraction) that brings its largest magnitude into
// [2^14, 2^15); the epilogue multiplies by the inverse scales of the output's row and column.
size_t tph_bytes(int rows, int K);
size_t tph_scale_ws_floats(int rows, int K);
void launch_tph_scales(const float* src, int rows, int K, int ld, float* row_scale, float* row_inv, float* col_scale,
                       float* col_inv, float* ws, hipStream_t st);
// several matrices in two launches (column scales always, row scales when row_scale != NULL); ws:
// tph_scale_batch_ws_floats(jobs, n) floats
constexpr int TPH_MAX_JOBS = 16;
struct TphScaleJob { const float* src; int rows, K, ld; float *row_scale, *row_inv, *col_scale, *col_inv; };
size_t tph_scale_batch_ws_floats(const TphScaleJob* jobs, int n);
void launch_tph_scales_batch(const TphScaleJob* jobs, int n, float* ws, hipStream_t st);
// scales from partial maxima somebody else took: rowpart [nrp][rows], colpart [ncp][K] (either pair may be NULL), one launch
void launch_tph_scales_from_parts(const float* rowpart, int nrp, int rows, float* row_scale, float* row_inv, const float* colpart,
                                  int ncp, int K, float* col_scale, float* col_inv, hipStream_t st);
void launch_fill(float* p, float v, int n, hipStream_t st);
// one pass over src [rows][K]: tpN = planes of src (scale per src row: row_scale[] or the constant rs), tpT = planes of its
// transpose (scale per src column: col_scale[] or cs); either may be NULL; colpart (or NULL): tp_split2_parts(rows) x K
// partial column sums of src, finished by launch_colsum_parts
// rowmap (or NULL): logical row i = physical row rowmap[i] of src (-1: zero row); rowmap2: the same for the columns from col2 on
void launch_tph_split2(const float* src, unsigned char* tpN, unsigned char* tpT, int rows, int K, int ld,
                       const float* row_scale, float rs, const float* col_scale, float cs, float* colpart, hipStream_t st,
                       const int* rowmap = nullptr, const int* rowmap2 = nullptr, int col2 = 0);
void launch_gather_rows(float* dst, const float* src, const int* map, int n, float fill, hipStream_t st);
struct GemmTPHDesc {
  const unsigned char* A;   // TPH of [>= M rows][K_A], starting at the first row block used
  const unsigned char* B;   // TPH of [>= N rows][K_B]
  float* C;
  int M, N, K;              // M, N multiples of 4 (row blocks past M / N read as zero), K = contraction length
  // K and the operands' k extents.  A step of the kernel is TWO k-blocks, so the sum runs over k in [0, Kc), Kc =
  // 32 * ceil(K / 32): whatever an operand holds in [K, Kc) (A: after its shift) ENTERS the product - the rest of a ragged
  // k-block and, when ceil(K/16) is odd, the whole k-block ceil(K/16) if it is < nkbA / nkbB.  Nothing from Kc on is read.
  // So either K covers the operand's extent (nkbA, nkbB <= ceil(K/16): every caller - the planes are written by
  // launch_tph_split2 for exactly K, which zero-fills the ragged tail) or the operand holds zeros in [K, Kc).
  // (tests/test_gpu_gemm_kernels.py: test_tph_contraction_runs_over_whole_steps)
  int nkbA, nkbB;           // k-blocks per row block in A / B: ceil(K_A/16), ceil(K_B/16)
  int ldc;
  int a_kshift;             // multiple of 16: A is read at k + a_kshift, zero outside [0, K_A)
  const float* bias;        // per-n, only with split_k == 1
  const float* a_inv;       // [M] inverse scales of A's rows
  const float* b_inv;       // [N] inverse scales of B's rows
  int split_k;              // > 1: partial slabs + reduction; needs ldc == N and no bias
  float* slabs;             // split_k * M * N floats
  int tile_rows;            // 0: gemm_tp_tile_rows(M); 192 / 256 forces the block tile (tools/gemmbench.hip)
  // nbatch == 2: a second product of the same shape in the same launch (the two directions' recurrent weight gradients):
  // its operands start a_bstride / b_bstride BYTES after A / B, its result c_bstride floats after C, its A shift is
  // a_kshift1.  With split_k > 1: c_bstride must be M * N (one reduction covers both) and slabs hold 2 * split_k * M * N.
  int nbatch;
  size_t a_bstride, b_bstride;
  int64_t c_bstride, ainv_bstride, binv_bstride;
  int a_kshift1;
  bool side;                // the 3-wave 128 x 192 instantiation that fits beside a persistent-recurrence workgroup
  const int* c_map;         // (or NULL) output row m goes to row c_map[m] of C (-1: dropped); nbatch == 1 only.  `side` has no
                            // scattering epilogue: with split_k == 1 it ignores c_map (row m -> row m); its reduction scatters
};
hipError_t gemm_tph_prepare();
int gemm_tph_pick_split(int M, int N, int K, int nbatch = 1);
void launch_gemm_tph(const GemmTPHDesc& g, hipStream_t st);

// ---- LSTM recurrence (lstm.hip) ----
struct LstmDims { int T, B, Bp, H, Hp, D; };   // D directions
// Contract of every recurrence launcher below and in the two sections that follow, on what is not computed
// (tests/test_gpu_rec_kernels.py holds each of them to it):
//   seq_len   Bp entries, 0 in the rows b >= B.  Frame t of row b is computed iff t < seq_len[b].  A row b < B may have
//             length 0 too (a stream slot without frames in a chunk: validate_chunk admits it, validate_batch does not):
//             every kernel treats it like a padded row, whatever state it carries.
//   forward   gates and cbuf of a frame that is not computed are neither written nor allowed into a result (gates may
//             hold anything there: the ragged input GEMM leaves them alone); out is +0 there, for every row b < Bp.
//   BPTT      gates, cbuf and dOut of such a frame may be loaded (unconditional loads) but never enter a result; dG is +0
//             there, for every row b < Bp.
//   units     j in [H, Hp): U's padded rows and columns and the padded gate columns of the input must be 0; c and out
//             are then exactly 0 there.  dOut must be 0 there too (it is: the layer above has zero weights for them);
//             dG is +0 there, on every path.  These columns of dG enter the weight- and bias-gradient passes of the
//             padded parameters, and the Adam sweep covers the padding: the gradient of a padded parameter must be
//             exactly 0 for the parameter to stay 0 (a sum of subnormals over T*B rows is enough to move it: Adam divides
//             by eps), and the requirement above that U's padding is 0 rests on that.  (The persistent BPTT's partial
//             sums carry their epoch in the last mantissa bit, so the dh it computes for a padded unit can be 32 x 2^-149:
//             it stores +0 in dG for the units j >= dm.H, and its rowpart / colpart are the maxima of what it stores.)
//             DESIGN.md §24; tests/test_gpu_padding.py, tests/test_gpu_rec_kernels.py.
// repack canonical U [Hp][N4] of every (layer,dir) into the forward / backward MFMA B-operand images
void launch_repack_u(const float* U, float* Uf, float* Ub, int Hp, hipStream_t st);
// One layer's buffers as the per-step kernels see a window of dm.T steps: a whole batch, a stream feed's chunk, or one
// window of a chunked batch (rows [k*W, (k+1)*W) of the layer's buffers with wlen[k] as its seq_len).
int lstm_bwd_partials(int Hp);   // partial sums a BPTT step hands to the next, per output
struct StepWindow {
  LstmDims dm;
  const float *Uf, *Ub;                 // [D] operand images of launch_repack_u
  float *hstate, *partial, *dcstate;    // two images each, handed launch to launch: h [D][Bp*Hp] (operand layout), partial sums
                                        // [D][lstm_bwd_partials(Hp)][Bp][Hp] of dh, dc [D][Bp][Hp]
  float *gates, *cbuf, *out;            // [T*Bp][..]: forward in place / out; BPTT reads gates and cbuf
  float* dg;                            // BPTT out: dG, frame indexed
  const float* dout;                    // BPTT in: the gradient from above
  const int* seq_len;
  float forget_bias;
  // NULL: the window starts a sequence, from an h image the forward runner zeroes itself.  Else step 0 runs in its carry
  // form: forward from the h image already in hstate[0] and c0 [D][Bp][Hp] (launch_stream_load_state, launch_lc_load_carry)
  // instead of zeros, and BPTT step 0 with the forget gate's derivative reading c0.  What BPTT step 0 leaves is then the
  // gradient with respect to the carried (h, c): dG x U^T in its partial sums, dc . f in its dc image.
  const float* c0;
};
// forward: steps [s0, s1), in order.  BPTT: steps s1-1 .. s0; the range that starts at the window's last step (s1 == dm.T)
// first zeroes the partial-sum and dc images that step reads - once per window, however the window is cut into ranges (an
// empty range enqueues nothing).  Ranges of one window run in order, with no other window between them.
void lstm_steps_fwd(const StepWindow& w, int s0, int s1, hipStream_t st);
void lstm_steps_bwd(const StepWindow& w, int s0, int s1, hipStream_t st);
// the dc image [D][Bp][Hp] BPTT step s of the window will read, and the images step s has written
struct StepLeft { float *partial, *dc; };
float* lstm_steps_dcin(const StepWindow& w, int s);
StepLeft lstm_steps_left(const StepWindow& w, int s);
// A stream session's feed as the kernels see it (nasr_stream.hip), per slot: rows held before the feed,
// new rows, rows the feed emits (without a look-ahead: 0, n, n).  Passed by value: a feed needs no upload of its own for them.
constexpr int LA_MAX_SLOTS = 64;
struct LaSlots { int held[LA_MAX_SLOTS], n[LA_MAX_SLOTS], emit[LA_MAX_SLOTS]; };
// one layer's forward stream state [S][2][H] (c, then h) -> step 0's h operand images [D][Bp*Hp] and c [D][Bp][Hp]:
// direction 0 from the state, the others, padded units and padded slots zero; and back from the first Hp of row
// (emit[b]-1)*Bp+b of out / cbuf [T*Bp][DH], DH = D*Hp (emit[b] = 0: untouched).  D = 1 loads one direction from a state:
// the kernel tests call it so, once per direction at an offset.
void launch_stream_load_state(const float* state, float* himg, float* cimg, int S, int H, int Bp, int Hp, hipStream_t st, int D = 1);
void launch_stream_save_state(const float* out, const float* cbuf, const LaSlots& sl, float* state, int S, int H, int Bp, int DH,
                              hipStream_t st);

// Latency-controlled training: the batch as the windows of a look-ahead session.
// Window k of an utterance of len frames holds frames [k*C, min(k*C + W, len)), W = C + R (or the batch's T when that is
// less: one window then); the first window that reaches
// the utterance's end is its last and emits all its rows, every earlier one emits its first C.  The windows of a batch lie on
// a virtual time axis of K windows x W rows: row (k*W + tl)*Bp + b.
struct LcGeom { int C, W, K, T, Bp; };   // K = lc_last_window(T) + 1 for the batch's T
__host__ __device__ inline int lc_last_window(int len, int C, int W) { return len <= W ? 0 : (len - W + C - 1) / C; }
__host__ __device__ inline int lc_window_rows(int len, int k, int C, int W) {
  if (len < 1 || k > lc_last_window(len, C, W)) return 0;
  return len - k * C < W ? len - k * C : W;
}
// what step 0 of window k starts from, as launch_stream_load_state writes it (the same kernel): direction 0 from row C-1 of
// window k-1 of out / cbuf (this layer's, [K*W*Bp][D*Hp]); zeros for window 0, the other directions and utterances without
// rows in window k (wlen [K][Bp])
void launch_lc_load_carry(const float* out, const float* cbuf, const int* wlen, int k, const LcGeom& g, float* himg, float* cimg,
                          int Hp, int D, hipStream_t st);
// behind step 0 of window k's BPTT: drow [Bp][DH] (row C-1 of window k-1 of dout) += the sum of direction 0's np partial
// sums, dcc [Bp][Hp] = its dcout; zeros for utterances without rows in window k (wlen_k [Bp]).  launch_lc_carry_dc adds dcc
// to the dcin [n = Bp*Hp] that step C-1 of window k-1 reads.
void launch_lc_carry_out(const float* part, int np, const float* dcs, const int* wlen_k, float* drow, float* dcc, int Bp, int Hp,
                         int DH, hipStream_t st);
void launch_lc_carry_dc(float* dcin, const float* dcc, int n, hipStream_t st);

// ---- row movers (rows.hip): features into the stack's rows, a look-ahead session's windows, a chunked batch's windows ----
// Frame skip: with skip s the network sees input frames 0, s, 2s, ... - n input frames are
// skip_frames(n, s) network frames.  The three feature movers below take T and seq_len in INPUT frames and write
// skip_frames(T, skip) x Bp rows: row t*Bp + b from input frame t*skip, zeros from the utterance's network length on.
__host__ __device__ inline int skip_frames(int n, int skip) { return (n + skip - 1) / skip; }
// seq_in [Bp] input lengths; NULL (skip 1 only): every row of the caller's is copied, padding included
void launch_pack_feats(const float* feats_bm, float* X0, int B, int Bp, int T, int F, int Fp, hipStream_t st, int skip = 1,
                       const int* seq_in = nullptr);
void launch_expand_context(const float* centre, const float* pad, const int* seq_len, float* X0, int B, int Bp, int T,
                           int ctx, int ncep, int Fp, hipStream_t st, int skip = 1);
// The same with SpecAugment masks on the centre frames (no counterpart in the reference): masks [B][nm] of
// {t0, tw, f0, fw}, utterance b's k-th time mask over frames [t0, t0 + tw) and its k-th frequency mask over columns
// [f0, f0 + fw) of each static_width-wide block of a frame; width 0 = no mask.  Masked centre values are 0, pads stay.
// Uses 2*ctx+1 + ncep bytes of dynamic LDS.
void launch_expand_context_masked(const float* centre, const float* pad, const int* seq_len, const int* masks, int nm,
                                  int static_width, float* X0, int B, int Bp, int T, int ctx, int ncep, int Fp,
                                  hipStream_t st, int skip = 1);
// A stream feed's kept rows: in [S][Tc][F] -> out [S][Tk][F], slot b's row j from input row first[b] + j*skip for
// j < kept[b] (kept[b] <= Tk and first[b] + (kept[b]-1)*skip < Tc), zeros behind them.  Tk >= 1.
struct SkipSlots { int first[LA_MAX_SLOTS], kept[LA_MAX_SLOTS]; };
void launch_skip_rows(const float* in, const SkipSlots& sk, float* out, int S, int Tc, int Tk, int F, int skip, hipStream_t st);
// Window assembly: pending row t of slot b is hold_in [S][R][F] row t (t < held) or fresh [S][Tc][F] row t - held; rows
// [0, P) of an emitting slot go to win [S][T][F] (zeros elsewhere; win NULL: nothing emits), rows [emit, P) to hold_out
// [S][R][F], which must not be hold_in.  rows = the largest P, >= 1.
void launch_la_window(const float* hold_in, const float* fresh, const LaSlots& sl, float* win, float* hold_out, int S, int R,
                      int Tc, int T, int rows, int F, hipStream_t st);
// src [T*Bp][F] by frame -> dst [K*W*Bp][F] by window row (zeros where wlen [K][Bp] gives a window no such row)
void launch_lc_gather(const float* src, const int* wlen, float* dst, const LcGeom& g, int F, hipStream_t st);
// the emitted rows of outv [K*W*Bp][DH] by frame into top [T*Bp][DH] (zeros from seq_len[b] on), and the transpose: doutv
// gets dtop's row in every emitted window row and zeros in the look-ahead rows and the rows no window has
void launch_lc_emit(const float* outv, const int* seq_len, float* top, const LcGeom& g, int DH, hipStream_t st);
void launch_lc_scatter(const float* dtop, const int* seq_len, const int* wlen, float* doutv, const LcGeom& g, int DH,
                       hipStream_t st);

// ---- persistent recurrence (lstm_persist.hip): one launch per layer pass, one XCD per (direction, utterance slice) ----
// the head of every resident kernel's control block (the first bytes of PersistCtl and WideCtl): placement and abort,
// served by join_xcd() / raise_error() of lstm_device.h
struct XcdCtl {                // device words, zeroed before every launch
  unsigned xcc_count[8];       // ticket per XCD: member index of a workgroup inside its XCD
  unsigned error;              // bit 0: a bounded spin gave up, bit 1: placement is not 32 workgroups on each of 8 XCDs,
                               // bit 2 (wide BPTT): dG left the fp16 range of its planes
  unsigned pad[23];            // (diagnostic build of tools/persistbench: the phase cycles of workgroup (0,0)'s wave 0)
};
static_assert(sizeof(XcdCtl) == 32 * sizeof(unsigned), "the control blocks' head is 32 words");
struct PersistCtl : XcdCtl {
  unsigned flags[8 * 128];     // per group: forward 32 words (one per member), BPTT 128 (member*4 + wave)
#if defined(NASR_PSTAMP) && NASR_PSTAMP
  unsigned stamps[256][12];    // diagnostic build only (tools/persistbench): wave 0's phase cycles of EVERY workgroup
#endif
};
bool persist_supported(int Hp);
size_t persist_image_floats(int Hp, bool bwd);   // floats of one direction's operand image
size_t persist_xch_floats(int Hp);               // floats of the exchange buffer (shared by forward and BPTT)
size_t persist_hx_bytes(int Hp);                 // its head, the forward kernel's h buffers: cleared before every forward launch
size_t persist_px_bytes();                       // the BPTT kernel's partial-sum buffers: cleared before every BPTT launch
hipError_t persist_prepare();                    // once per process: raise the kernels' dynamic-LDS limit
// all n (layer, direction) matrices in one launch: matrix k is P + offs[k], its images Upf + k*image_floats(fwd) / Upb + k*...(bwd)
constexpr int PERSIST_MAX_MATS = 16;
// col_scale (or NULL): [n][4*Hp] power-of-two scales of every matrix's columns -> the forward image holds two fp16 planes
void launch_repack_persist(const float* P, const int64_t* offs, int n, float* Upf, float* Upb, int Hp, const float* col_scale,
                           hipStream_t st);
// Upf/Upb: [D] images of this layer; xch: persist_xch_floats(Hp) floats; ctl: one PersistCtl (zeroed by the launcher);
// sticky: host-mapped word that receives the error code of an aborted launch (or NULL); fault: device float set to 1
// by an aborted launch (or NULL) - the engine keeps it behind the gradients so that it is all-reduced with them
// cinv (or NULL): [D][4*Hp] inverse column scales of this layer's matrices = the fp16 form of the forward image
void launch_lstm_persist_fwd(const LstmDims& dm, const float* Upf, const float* cinv, float* gates, float* cbuf,
                             float* out, const int* seq_len, float* xch, PersistCtl* ctl, unsigned* sticky, float* fault,
                             float forget_bias, hipStream_t st, bool ctl_zeroed = false);   // ctl_zeroed: the caller cleared *ctl AND the first persist_hx_bytes of xch
void launch_lstm_persist_bwd(const LstmDims& dm, const float* Upb, const float* gates, float* dgbuf, const float* cbuf,
                             const float* dout, const int* seq_len, float* xch, PersistCtl* ctl, unsigned* sticky,
                             float* fault, hipStream_t st, bool ctl_zeroed = false, float* rowpart = nullptr,
                             float* colpart = nullptr, bool lean = false);   // ctl_zeroed: the caller cleared *ctl AND persist_px_bytes of xch
// rowpart [D*32][T*Bp], colpart [8/D][D*4Hp] (or NULL): partial maxima of |dG| per frame row / per gate column, written by the
// kernel's memory wave; launch_tph_scales_from_parts turns them into operand scales (persist_dgmax_floats sizes both)
// lean: at Hp = 512 the launch declares only the 24 KB of LDS it uses instead of 96 KB, so that another kernel's workgroup
// can share its CUs (the weight gradients of the side stream)
size_t persist_dgmax_floats(int T, int Bp, int Hp, int D);

// ---- wide persistent forward recurrence (lstm_wide.hip): Hp = 2048, one launch per direction over all 256 CUs ----
struct WideCtl : XcdCtl {
  unsigned stamps[160];        // diagnostic build (NASR_WSTAMP, tools/widebench): phase cycles of two workgroups' waves
};
struct WideGeom {
  int T, Bp, Hp, D, d;
  int inject;                  // test hook (NASR_WIDE_FAULT=s): workgroup (0,0) treats the poll of step s as timed out
  int scale_shift;             // test hook (NASR_WIDE_SCALE_SHIFT): added to the exponent of the BPTT's dG scales
  float* fault;
};
bool wide_supported(int Hp, int Bp);
size_t wide_image_bytes(int Hp);     // one direction's operand image
size_t wide_hx_bytes(int Bp);        // h exchange buffer
size_t wide_part_bytes(int Bp);      // partial-sum exchange buffer
hipError_t wide_prepare();           // once per process: raise the kernels' dynamic-LDS limit
// U [Hp][4Hp] canonical, cs [4Hp] power-of-two column scales -> Uw (wide_image_bytes)
void launch_repack_wide(const float* U, const float* cs, void* Uw, int Hp, hipStream_t st);
// direction d of one layer: Uw / cinv ([4Hp], 1 / cs) of that direction; gates/cbuf/out frame-indexed as everywhere
void launch_lstm_wide_fwd(const LstmDims& dm, int d, const void* Uw, const float* cinv, float* gates, float* cbuf,
                          float* out, const int* seq_len, void* hx, float* part, WideCtl* ctl, unsigned* sticky,
                          float* fault, float forget_bias, hipStream_t st);

// BPTT of the same layer: Uwb = the backward image (U^T fragments under per-row scales rs [Hp]; rinv = 1 / rs), srow [D][Bp]
// = largest |dOut| per (direction, utterance) from launch_wide_row_scales (the kernel derives its power-of-two dG scale); inbox = the forward kernel's partial-sum
// buffer (wide_part_bytes), px = wide_px_bytes
size_t wide_px_bytes(int Bp);
void launch_repack_wide_bwd(const float* U, const float* rs, void* Uwb, int Hp, hipStream_t st);
void launch_wide_row_scales(const LstmDims& dm, const float* dout, const int* seq_len, float* srow, hipStream_t st);
void launch_lstm_wide_bwd(const LstmDims& dm, int d, const void* Uwb, const float* rinv, const float* srow,
                          const float* gates, float* dgbuf, const float* cbuf, const float* dout, const int* seq_len,
                          float* inbox, void* px, WideCtl* ctl, unsigned* sticky, float* fault, hipStream_t st);

// ---- DeepSpeech dense stages (dense.hip): clipped ReLU + hash-defined dropout, in place ----
void launch_dense_act(float* z, int R, int Bp, int B, int W, int ld, float clip, float p, uint32_t seed, uint32_t counter,
                      int stage, hipStream_t st);
void launch_dense_act_bwd(float* dy, const float* y, int64_t n, float clip, float p, hipStream_t st);

// ---- CTC (ctc.hip) ----
// Contract of the launchers below, on what is read, what is ignored and what is written where
// (tests/test_gpu_ctc_kernels.py holds each of them to it, launch by launch against fp64):
//   shapes    B in [1,64], Bp = round_up(B,16), C >= 2, Cp = round_up(C,32), Lmax >= 1 with KS = ctc_states_per_lane(Lmax) <= 16,
//             T' * Bp * Cp * 4 < 2^32 (the walks and the alignment gather at 32-bit byte offsets; ensure_ctc_buffers, align_run
//             and the distillation entry refuse more).  seq_len [Bp]: in [1,T'] for b < B.  labels [B][Lmax] with ids in
//             [0, C-2] in the first label_len[b] <= Lmax entries of a row, feasible in seq_len[b] frames (validate_batch).
//   read      logits (t,b,c) with b < B, t < seq_len[b], c < C; the first label_len[b] entries of a label row; cstart / cpos
//             of the rows b < B.  Nothing else enters a result: the columns [C,Cp), the rows b >= B, the frames
//             t >= seq_len[b] and the label entries from label_len[b] on may hold anything (NaN, any in-range id), and so
//             may every workspace (alpha, beta, aoff, boff, lprobs, goff, the greedy argmax) before the launch.
//   logz      written at the rows (t,b) with b < B and t < seq_len[b]; every other row stays untouched.
//   nll,logp  entries b < B are written, nothing behind them.
//   gradient  in place over all T' * Bp rows and Cp columns: d(mean nll)/dlogits * scale where the logit is read, +0 in the
//             columns [C,Cp), the rows b >= B and the frames t >= seq_len[b].
//   greedy    ids [B][T'] hold lens[b] entries per row; the rest of a row stays untouched.
//   placement a result of utterance b depends on its own logits, label and lengths alone: not on its slot, on B, on T' or on
//             the stride Lmax (inside one KS).  Two runs give the same bits (fixed summation orders, no atomics).
struct CtcDims {
  int Tp;      // logit frames T'
  int B, Bp, C, Cp, Lmax;
  int KS;      // states per lane: ctc_states_per_lane(Lmax)
  int Tws;     // rows of the alpha/beta workspace per utterance (T + 8: a group of up to 8 frames may run past the last one)
  // workspaces of the engineered lattice (ctc.hip (2b)), or NULL (the plain one only):
  float* lprobs = nullptr;  // [T'][Bp][Cp] emission rows log2 y(t,k) (launch_ctc_logz writes them)
  double* goff = nullptr;   // [B][2][ctc_group_rows(Tws)] column offsets per walk and group of 4 frames
};
// The lattice kernels' instantiation for a label array of width Lmax: ceil((2 Lmax + 1) / 64) states per lane, two at least
// (a step then never reaches past the neighbour lane), rounded up to one of 2 .. 8, 12, 16.  More than 16 (Lmax > 511):
// no instantiation - the caller reports it.
constexpr int ctc_states_per_lane(int Lmax) {
  const int KS = (2 * (Lmax > 0 ? Lmax : 0) + 1 + 63) / 64;
  return KS <= 1 ? 2 : KS <= 8 ? KS : KS <= 12 ? 12 : KS <= 16 ? 16 : KS;
}
// column offsets the engineered lattice keeps per utterance and walk: one per group of 4 frames of the Tws workspace rows
// (group 0 = the start column) and room for the masked last group
constexpr int ctc_group_rows(int Tws) { return Tws / 4 + 3; }
void launch_ctc_logz(const CtcDims& d, const float* logits, const int* seq_len, float* logz, hipStream_t st);
void launch_ctc_alpha_beta(const CtcDims& d, const float* logits, const float* logz, const int* labels,
                           const int* label_len, const int* seq_len, float* alpha, float* beta, double* aoff,
                           double* boff, float* nll, double* logp, hipStream_t st);
// in place: logits -> d(mean nll)/dlogits
// cstart [B][C+1], cpos [B][Lmax]: the label positions of every utterance sorted by class (ascending inside a class)
void launch_ctc_grad(const CtcDims& d, float* logits, const float* logz, const int* label_len, const int* seq_len,
                     const int* cstart, const int* cpos, const float* alpha, const float* beta, const double* aoff,
                     const double* boff, const double* logp, float scale, hipStream_t st);
// One utterance's cstart [C+1] / cpos [>= L] from its label (L ids in [0, C-2]): a counting sort on the host - the fixed
// summation order of ctc_grad.  cstart must come in zeroed; fill: scratch of the caller's, resized here.
inline void ctc_class_positions(const int32_t* label, int L, int C, int32_t* cstart, int32_t* cpos, std::vector<int32_t>& fill) {
  fill.resize((size_t)C);
  for (int i = 0; i < L; ++i) cstart[label[i] + 1] += 1;
  for (int c = 0; c < C; ++c) cstart[c + 1] += cstart[c];
  for (int c = 0; c < C; ++c) fill[c] = cstart[c];
  for (int i = 0; i < L; ++i) cpos[fill[label[i]]++] = i;
}
void launch_mean(const float* v, int n, float* out, hipStream_t st);
void launch_greedy(const CtcDims& d, const float* logits, const int* seq_len, int* argmax_ws, int* ids, int* lens,
                   hipStream_t st);

// forced alignment (ctc.hip (4)): the best path of every utterance through its CTC lattice over the raw logits.
// path [B][T'] = the state of every frame (-1 from seq_len[b] on), score [B] = sum over the path of x - logZ (fp64).
// Uses d.Tp, B, Bp, C, Cp, Lmax (the stride of `labels`, >= 1); F = the batch's longest seq_len.  Back-pointers stay in LDS when
// ctc_align_bp_in_lds(F, Lmax); otherwise bpws must hold ctc_align_ws_words(B, F, Lmax) words.  < 0: the logits are too
// large for 32-bit offsets (-1), or bpws is missing (-2); nothing is launched then.
bool ctc_align_bp_in_lds(int F, int L);
size_t ctc_align_ws_words(int B, int F, int L);
int launch_ctc_align(const CtcDims& d, int F, const float* logits, const float* logz, const int* labels, const int* label_len,
                     const int* seq_len, unsigned* bpws, int* path, double* score, hipStream_t st);

// distillation term (ctc.hip (5)) over student and teacher logits [T'*Bp][Cp]; uses d.Tp, B, Bp, C, Cp.
// rows: dgrad [T'*Bp][Cp] = weight * tau * (q - p) / B (0 on rows outside the batch and columns from C on), klrow [T'*Bp]
// the rows' KL(p || q), kd [B] their sum per utterance in fp64 and a fixed order.  combine: parts = {CTC = *loss,
// KD = tau^2 mean_b kd[b]}, *loss = (1 - weight) CTC + weight KD, *fault takes a non-zero *teacher_fault.  add: grad += dgrad.
void launch_distill_rows(const CtcDims& d, const float* student, const float* teacher, const int* seq_len, float weight,
                         float tau, float* dgrad, float* klrow, double* kd, hipStream_t st);
void launch_distill_combine(const double* kd, int B, float weight, float tau, float* loss, float* parts,
                            const float* teacher_fault, float* fault, hipStream_t st);
void launch_distill_add(const CtcDims& d, float* grad, const float* dgrad, hipStream_t st);

// ---- optimiser / reductions (optim.hip) ----
// Adam's step count and the step size derived from it, on the device: a launch whose `fault` word (device float, or NULL)
// is non-zero is a no-op AND leaves the count alone, so a void step never enters the bias correction.
struct AdamDev { long long step; float lr_t; int applied; };
// Parameter averaging (nasr_set_ema): the number of updates applied so far and omd = (float)(1 - d_n) of the step in flight,
// d_n = min(decay, (1 + n) / (10 + n)), advanced on the device wherever Adam's count is - never by a void or skipped step.
struct EmaDev { long long updates; float omd; };
constexpr int ADAM_MAX_BLOCKS = 2048;   // the grid of the Adam and swap sweeps; above 2048 * 256 float4s their loops go round again
// e: the average of p, updated in the same sweep from `ema` and `decay`, or NULL: the sweep without it
void launch_adam(float* p, float* m, float* v, const float* g, int64_t n, AdamDev* state, float lr, float beta1, float beta2,
                 float eps, float gscale, const float* fault, float* e, EmaDev* ema, float decay, hipStream_t st);
void launch_swap16(float* a, float* b, int64_t n, hipStream_t st);   // the contents of a and b change places (n % 4 == 0)
// Global-norm clipping (nasr_set_grad_clip): what the second stage of the norm decides for the step, on the device.  s is
// the multiplier the Adam pass reads (grad_scale * coef); skip = 1: the norm was not finite, the step touches nothing.
// window_max_norm .. skipped are the window nasr_get_grad_clip_stats(reset) clears.
struct ClipDev { double last_norm; float last_coef, s; int skip, pad; double window_max_norm; long long steps, clipped, skipped; };
constexpr int GRAD_SUMSQ_MAX_BLOCKS = 1024;
int grad_sumsq_blocks(int64_t n);   // workgroups (= partial sums) of the norm's first stage: a function of n alone
// launch_adam behind the norm of g: `part` holds GRAD_SUMSQ_MAX_BLOCKS doubles.  max_norm > 0 or +inf.
void launch_adam_clipped(float* p, float* m, float* v, const float* g, int64_t n, AdamDev* state, ClipDev* clip, double* part,
                         float lr, float beta1, float beta2, float eps, float gscale, float max_norm, const float* fault,
                         float* e, EmaDev* ema, float decay, hipStream_t st);
// out[n] = sum_r M[r*ld + n], deterministic two-stage; ws holds 32*N floats
void launch_colsum(const float* M, int R, int N, int ld, float* out, float* ws, hipStream_t st);
void launch_colsum_parts(const float* part, int nparts, int N, float* out, hipStream_t st);   // out[n] = sum_k part[k][n]
void launch_reduce_slabs(const float* slabs, int S, int64_t n, float* out, hipStream_t st);
void launch_reduce_slabs_rows(const float* slabs, int S, int M, int N, int ldc, const int* map, float* out, hipStream_t st);
// diagnostics: nblocks x 256 threads sweep buf[0..n) `passes` times with 16-byte loads / stores, data unchanged
void launch_ring_standin(float* buf, int64_t n, int nblocks, int passes, hipStream_t st);

}  // namespace nasr
